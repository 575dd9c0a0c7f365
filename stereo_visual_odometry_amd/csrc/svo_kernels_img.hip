// svo_kernels_img.hip — frame bookkeeping, ingest, pyrDown, FAST-9/16 + NMS, bucketing, compaction.
// gfx950 (wave64).  All integer / byte work: HBM-bound by design, no MFMA.
//
// Behaviour follows the reference call sites (cited per kernel); the arithmetic of the OpenCV
// functions they call is restated independently, not translated.
#include "svo_internal.hpp"
#include "svo_pyr_walk.hpp"
#include <type_traits>

// cv::borderInterpolate(i, n, BORDER_REFLECT_101) for any i: reflect about the first and the last pixel until i lies inside (the
// rule repeats with period 2n - 2).  A level narrower or shorter than the border pad needs more than one fold: the LK border of
// k_pad_pyramid reaches up to pad pixels out.  Every other caller stays within one fold of its level for every byte it keeps (the
// pyrDown taps reach 2 pixels out); the tile positions beyond a level's edge get some in-range pixel too, and are never stored.
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n <= 1) return 0;
    while ((unsigned)i >= (unsigned)n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

// ------------------------------------------------------------------------------------------------
// Rectification (svo.h, svo_set_rectification_maps): cv::remap(raw, out, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) with a
// CV_16SC2 + CV_16UC1 map, the step image_geometry::PinholeCameraModel::rectifyImage runs to make image_rect.  One output byte
// of channel c: integer position (x0, y0) = map1, fractions fx = map2 & 31, fy = (map2 >> 5) & 31 (OpenCV masks map2 to
// INTER_TAB_SIZE2 - 1 as well); the four 15-bit OpenCV weights are 32 x the integer products below, so
//   out = ((32-fx)(32-fy) p00 + fx(32-fy) p01 + (32-fx) fy p10 + fx fy p11 + 512) >> 10,
// a tap outside the raw image reads 0.  Every tap is bounds-checked before it is loaded: any map is safe.
// ------------------------------------------------------------------------------------------------
template <int CN>
__device__ __forceinline__ void remap_px(const uint8_t* __restrict__ raw, int stride, int rw, int rh, short2 p, unsigned f, uint8_t* out) {
    const int x0 = p.x, y0 = p.y, fx = f & 31, fy = (f >> 5) & 31;
    const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
    const bool x0in = (unsigned)x0 < (unsigned)rw, x1in = (unsigned)(x0 + 1) < (unsigned)rw;
    const bool y0in = (unsigned)y0 < (unsigned)rh, y1in = (unsigned)(y0 + 1) < (unsigned)rh;
    const ptrdiff_t o00 = (ptrdiff_t)y0 * stride + (ptrdiff_t)x0 * CN;
#pragma unroll
    for (int c = 0; c < CN; c++) {
        const int p00 = (y0in && x0in) ? raw[o00 + c] : 0, p01 = (y0in && x1in) ? raw[o00 + CN + c] : 0;
        const int p10 = (y1in && x0in) ? raw[o00 + stride + c] : 0, p11 = (y1in && x1in) ? raw[o00 + stride + CN + c] : 0;
        out[c] = (uint8_t)((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 512) >> 10);
    }
}
// the maps of (camera, sequence) of the frame being ingested: [W*H] short2, then [W*H] u16
__device__ __forceinline__ const short2* rect_map1(const DevBuffers& d, int cam, int seq) {
    return reinterpret_cast<const short2*>(d.rmap[cam * d.B + seq]);
}
__device__ __forceinline__ const uint16_t* rect_map2(const DevBuffers& d, int cam, int seq) {
    return reinterpret_cast<const uint16_t*>(d.rmap[cam * d.B + seq] + (size_t)4 * d.geom.W * d.geom.H);
}

// ------------------------------------------------------------------------------------------------
// Input formats (svo.h, svo_set_input_format): the grey byte of a colour or YUV 4:2:2 pixel, what cv_bridge::toCvCopy(img, MONO8)
// hands the reference (stereo_vo.cpp:6-14).  BPP = bytes per pixel: 3 / 4 weigh the first three bytes (the
// order of the weights in g makes it BGR or RGB, the fourth byte is never used), 2 picks the Y byte.  g is uniform: scalar registers.
// ------------------------------------------------------------------------------------------------
struct __attribute__((packed, aligned(1))) UD { unsigned v; };          // a dword at any byte address
struct __attribute__((packed, aligned(1))) UD2 { unsigned v[2]; };
struct __attribute__((packed, aligned(1))) UD4 { unsigned v[4]; };
typedef short grey_s2 __attribute__((ext_vector_type(2)));
// one pixel at p (BPP bytes, all inside the caller's row)
template <int BPP>
__device__ __forceinline__ unsigned grey_px(const uint8_t* __restrict__ p, const GreyIn& g) {
    if constexpr (BPP == 2) return p[g.yoff];
    else return ((unsigned)p[0] * g.w0 + (unsigned)p[1] * g.w1 + (unsigned)p[2] * g.w2 + g.rnd) >> g.shift;
}
// (byte0, byte1) as a 16-bit pair (one v_perm_b32 by the caller) and byte2: v_dot2_i32_i16 against the packed weight pair, seeded
// with the 24-bit multiply-add of the third channel and the rounding term.  Weights are < 2^15 and the sum < 2^31: exact.
__device__ __forceinline__ unsigned grey_w3(unsigned pair, unsigned third, unsigned wpair, const GreyIn& g) {
    const int seed = (int)(__umul24(third, (unsigned)g.w2) + (unsigned)g.rnd);
    return (unsigned)__builtin_amdgcn_sdot2(__builtin_bit_cast(grey_s2, pair), __builtin_bit_cast(grey_s2, wpair), seed, false) >> g.shift;
}
// FOUR consecutive pixels at p (4 BPP bytes, all inside the caller's row) as one dword of grey bytes: unaligned dword loads only —
// three dwords (BPP 3), one dwordx4 (BPP 4), one dwordx2 and one v_perm_b32 (BPP 2)
template <int BPP>
__device__ __forceinline__ unsigned grey4(const uint8_t* __restrict__ p, const GreyIn& g) {
    if constexpr (BPP == 2) {
        const UD2 q = *reinterpret_cast<const UD2*>(p);
        return __builtin_amdgcn_perm(q.v[1], q.v[0], g.yoff ? 0x07050301u : 0x06040200u);
    } else {
        const unsigned wpair = (unsigned)g.w0 | ((unsigned)g.w1 << 16);
        unsigned y0, y1, y2, y3;
        if constexpr (BPP == 3) {
            const unsigned a = reinterpret_cast<const UD*>(p)->v, b = reinterpret_cast<const UD*>(p + 4)->v, c = reinterpret_cast<const UD*>(p + 8)->v;
            y0 = grey_w3(__builtin_amdgcn_perm(a, a, 0x0c010c00u), (a >> 16) & 255u, wpair, g);      // bytes 0 1 | 2
            y1 = grey_w3(__builtin_amdgcn_perm(b, a, 0x0c040c03u), (b >> 8) & 255u, wpair, g);       // bytes 3 4 | 5
            y2 = grey_w3(__builtin_amdgcn_perm(b, b, 0x0c030c02u), c & 255u, wpair, g);              // bytes 6 7 | 8
            y3 = grey_w3(__builtin_amdgcn_perm(c, c, 0x0c020c01u), c >> 24, wpair, g);               // bytes 9 10 | 11
        } else {
            const UD4 q = *reinterpret_cast<const UD4*>(p);
            y0 = grey_w3(__builtin_amdgcn_perm(q.v[0], q.v[0], 0x0c010c00u), (q.v[0] >> 16) & 255u, wpair, g);
            y1 = grey_w3(__builtin_amdgcn_perm(q.v[1], q.v[1], 0x0c010c00u), (q.v[1] >> 16) & 255u, wpair, g);
            y2 = grey_w3(__builtin_amdgcn_perm(q.v[2], q.v[2], 0x0c010c00u), (q.v[2] >> 16) & 255u, wpair, g);
            y3 = grey_w3(__builtin_amdgcn_perm(q.v[3], q.v[3], 0x0c010c00u), (q.v[3] >> 16) & 255u, wpair, g);
        }
        return y0 | (y1 << 8) | (y2 << 16) | (y3 << 24);                 // every y is <= 255: the weights sum to 2^shift
    }
}
// remap_px<1> of a raw frame in the format g: each of the four taps is converted to grey first (image_mono -> image_rect), a tap
// outside the raw image is 0, then the bilinear formula above
template <int BPP>
__device__ __forceinline__ void remap_grey_px(const uint8_t* __restrict__ raw, int stride, int rw, int rh, short2 p, unsigned f, const GreyIn& g, uint8_t* out) {
    const int x0 = p.x, y0 = p.y, fx = f & 31, fy = (f >> 5) & 31;
    const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
    const bool x0in = (unsigned)x0 < (unsigned)rw, x1in = (unsigned)(x0 + 1) < (unsigned)rw;
    const bool y0in = (unsigned)y0 < (unsigned)rh, y1in = (unsigned)(y0 + 1) < (unsigned)rh;
    const uint8_t* t = raw + (ptrdiff_t)y0 * stride + (ptrdiff_t)x0 * BPP;
    const int p00 = (y0in && x0in) ? (int)grey_px<BPP>(t, g) : 0, p01 = (y0in && x1in) ? (int)grey_px<BPP>(t + BPP, g) : 0;
    const int p10 = (y1in && x0in) ? (int)grey_px<BPP>(t + stride, g) : 0, p11 = (y1in && x1in) ? (int)grey_px<BPP>(t + stride + BPP, g) : 0;
    *out = (uint8_t)((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 512) >> 10);
}
// the kernel instantiation of a run-time bytes-per-pixel count (2, 3 or 4; the host checked it): f(std::integral_constant<int, BPP>)
template <typename F>
static void with_bpp(int bpp, F&& f) {
    if (bpp == 2) f(std::integral_constant<int, 2>{}); else if (bpp == 3) f(std::integral_constant<int, 3>{}); else f(std::integral_constant<int, 4>{});
}

// svo_convert_gray: a thread per four pixels of a row (grey4 where all four exist, grey_px for a row's last one to three)
template <int BPP>
__global__ __launch_bounds__(256) void k_convert_gray(GreyIn g, const uint8_t* __restrict__ src, int w, int h, int stride, uint8_t* __restrict__ out) {
    const int qpr = (w + 3) >> 2, total = qpr * h;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int y = i / qpr, x = 4 * (i - y * qpr);
        const uint8_t* p = src + (size_t)y * stride + (size_t)x * BPP;
        uint8_t* o = out + (size_t)y * w + x;
        if (x + 4 <= w) { UD u; u.v = grey4<BPP>(p, g); *reinterpret_cast<UD*>(o) = u; }
        else for (int k = 0; x + k < w; k++) o[k] = (uint8_t)grey_px<BPP>(p + k * BPP, g);
    }
}
void launch_convert_gray(const GreyIn& g, const uint8_t* src, int w, int h, int stride, uint8_t* out, hipStream_t st) {
    int gx = (((w + 3) >> 2) * h + 255) / 256; if (gx > 4096) gx = 4096;
    with_bpp(g.bpp, [&](auto b) { hipLaunchKernelGGL(k_convert_gray<decltype(b)::value>, dim3(gx), dim3(256), 0, st, g, src, w, h, stride, out); });
}

// ------------------------------------------------------------------------------------------------
// CLAHE (svo.h, svo_set_clahe): two launches in front of a frame's ingest.  The LUTs need the whole image before the first pixel
// can be written, so nothing here is fused into the tile fills: k_clahe_lut builds one tile's LUT per block, k_clahe_apply
// interpolates four LUTs per pixel into a packed mono8 staging frame, which the frame's unchanged mono8 ingest then reads.
// BPP 1 reads the caller's bytes as they are; 2 / 3 / 4 convert through grey_px / grey4.
// ------------------------------------------------------------------------------------------------
template <int BPP>
__device__ __forceinline__ unsigned clahe_px(const uint8_t* __restrict__ p, const GreyIn& g) {
    if constexpr (BPP == 1) return p[0]; else return grey_px<BPP>(p, g);
}
template <int BPP>
__device__ __forceinline__ unsigned clahe_px4(const uint8_t* __restrict__ p, const GreyIn& g) {
    if constexpr (BPP == 1) return reinterpret_cast<const UD*>(p)->v; else return grey4<BPP>(p, g);
}
// One block per (tile, camera, launched sequence): per-wave histograms in LDS (LDS atomics), merged one bin per thread, clipped,
// redistributed, prefix-summed, scaled.  Only a tile that touches the extension computes REFLECT_101 indices (one fold: the host
// rejected an extension beyond w - 1 / h - 1); an interior tile takes four pixels per thread from unaligned dword loads.
// The redistribution loop of the definition visits bins 0, step, 2 step ... while residual lasts: bin t gets its + 1 when
// t % step == 0 and t / step < residual — the same bins, one thread each.
template <int BPP>
__global__ __launch_bounds__(256) void k_clahe_lut(ClaheArgs a) {
    __shared__ unsigned hist[4][256];
    __shared__ unsigned part[2][4];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int tile = blockIdx.x, cam = blockIdx.y, seq = a.act ? a.act[blockIdx.z] : (int)blockIdx.z;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
#pragma unroll
    for (int k = 0; k < 4; k++) hist[k][t] = 0;
    __syncthreads();
    const uint8_t* __restrict__ src = a.srcs[cam * a.B + seq];
    const int x0 = tx * a.tw, y0 = ty * a.th;
    const bool inside = x0 + a.tw <= a.w && y0 + a.th <= a.h;
    const int qpr = (a.tw + 3) >> 2, total = qpr * a.th;
    unsigned* const my = hist[wave];
    for (int i = t; i < total; i += 256) {
        const int r = i / qpr, x = 4 * (i - r * qpr);
        const int ey = y0 + r, sy = ey < a.h ? ey : 2 * a.h - 2 - ey;
        const uint8_t* row = src + (size_t)sy * a.stride;
        if (inside && x + 4 <= a.tw) {
            const unsigned q = clahe_px4<BPP>(row + (size_t)(x0 + x) * BPP, a.g);
            atomicAdd(&my[q & 255u], 1u); atomicAdd(&my[(q >> 8) & 255u], 1u); atomicAdd(&my[(q >> 16) & 255u], 1u); atomicAdd(&my[q >> 24], 1u);
        } else {
            for (int k = 0; k < 4 && x + k < a.tw; k++) {
                const int ex = x0 + x + k, sx = ex < a.w ? ex : 2 * a.w - 2 - ex;
                atomicAdd(&my[clahe_px<BPP>(row + (size_t)sx * BPP, a.g)], 1u);
            }
        }
    }
    __syncthreads();
    unsigned hv = hist[0][t] + hist[1][t] + hist[2][t] + hist[3][t];
    if (a.clip > 0) {
        const unsigned clip = (unsigned)a.clip;
        unsigned ex = hv > clip ? hv - clip : 0u;
        hv = hv > clip ? clip : hv;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ex += __shfl_xor(ex, o);
        if (lane == 0) part[0][wave] = ex;
        __syncthreads();
        const unsigned clipped = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        const unsigned batch = clipped >> 8, residual = clipped & 255u;
        hv += batch;
        if (residual > 0) {
            const unsigned step = 256u / residual;                    // >= 1: residual <= 255
            if (t % step == 0 && t / step < residual) hv++;
        }
    }
    unsigned s = hv;                                                  // inclusive scan over the 256 bins
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned n = __shfl_up(s, o); if (lane >= o) s += n; }
    if (lane == 63) part[1][wave] = s;
    __syncthreads();
    for (int k = 0; k < wave; k++) s += part[1][k];
    float f = rintf(__fmul_rn((float)s, a.scale));
    f = f < 0.f ? 0.f : (f > 255.f ? 255.f : f);
    a.lut[((size_t)(seq * a.ncam + cam) * (a.tiles_x * a.tiles_y) + tile) * 256 + t] = (uint8_t)(int)f;
}
// A block takes up to CLAHE_ROWS pixel rows of one BAND: the rows whose ty1 = floor(y inv_th - 0.5) is blockIdx.y - 1, which all
// interpolate between the same two LUT rows — staged in LDS, 2 tiles_x 256 bytes.  The band's rows are found by the definition's own
// f32 expression, evaluated for a candidate range two rows wider than the exact one on both sides; a row of another band is skipped.
// Each lane handles four pixels of a row: converts them, looks up four LUTs per pixel, interpolates (every f32 operation rounded on
// its own, in the definition's order) and stores one dword.
#define CLAHE_ROWS 8
template <int BPP>
__global__ __launch_bounds__(256) void k_clahe_apply(ClaheArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t L[2][16 * 256];
    const int t = threadIdx.x, band = blockIdx.y;
    const int b = blockIdx.z / a.ncam, cam = blockIdx.z - b * a.ncam, seq = a.act ? a.act[b] : b;
    const int lo = max((band - 1) * a.th + a.th / 2 - 2, 0), hi = min(band * a.th + (a.th + 1) / 2 + 2, a.h);
    const int r0 = lo + blockIdx.x * CLAHE_ROWS;
    if (r0 >= hi) return;
    const int rowb = a.tiles_x * 256;
    const uint8_t* lut = a.lut + (size_t)(seq * a.ncam + cam) * ((size_t)rowb * a.tiles_y);
    const unsigned* la = reinterpret_cast<const unsigned*>(lut + (size_t)max(band - 1, 0) * rowb);
    const unsigned* lb = reinterpret_cast<const unsigned*>(lut + (size_t)min(band, a.tiles_y - 1) * rowb);
    for (int i = t; i < rowb / 4; i += 256) {
        reinterpret_cast<unsigned*>(L[0])[i] = la[i];
        reinterpret_cast<unsigned*>(L[1])[i] = lb[i];
    }
    __syncthreads();
    const uint8_t* __restrict__ src = a.srcs[cam * a.B + seq];
    uint8_t* __restrict__ out = a.out + (size_t)(cam * a.B + seq) * a.pitch;
    const int qpr = (a.w + 3) >> 2, total = qpr * CLAHE_ROWS;
    for (int i = t; i < total; i += 256) {
        const int r = i / qpr, y = r0 + r, x = 4 * (i - r * qpr);
        if (y >= hi) break;
        const float tyf = __fsub_rn(__fmul_rn((float)y, a.inv_th), 0.5f), ty1f = floorf(tyf);
        if ((int)ty1f != band - 1) continue;
        const float ya = __fsub_rn(tyf, ty1f), ya1 = __fsub_rn(1.0f, ya);
        const uint8_t* p = src + (size_t)y * a.stride + (size_t)x * BPP;
        uint8_t* o = out + (size_t)y * a.w + x;
        const bool full = x + 4 <= a.w;
        const unsigned q = full ? clahe_px4<BPP>(p, a.g) : 0u;
        unsigned res4 = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!full && x + k >= a.w) break;
            const unsigned v = full ? (q >> (8 * k)) & 255u : clahe_px<BPP>(p + k * BPP, a.g);
            const float txf = __fsub_rn(__fmul_rn((float)(x + k), a.inv_tw), 0.5f), tx1f = floorf(txf);
            const float xa = __fsub_rn(txf, tx1f), xa1 = __fsub_rn(1.0f, xa);
            const int tx1 = (int)tx1f;
            const int c1 = min(max(tx1, 0), a.tiles_x - 1) * 256 + (int)v, c2 = min(tx1 + 1, a.tiles_x - 1) * 256 + (int)v;   // (the upper clamp of tx1 never binds: x < tiles_x tw)
            const float top = __fadd_rn(__fmul_rn((float)L[0][c1], xa1), __fmul_rn((float)L[0][c2], xa));
            const float bot = __fadd_rn(__fmul_rn((float)L[1][c1], xa1), __fmul_rn((float)L[1][c2], xa));
            float res = rintf(__fadd_rn(__fmul_rn(top, ya1), __fmul_rn(bot, ya)));
            res = res < 0.f ? 0.f : (res > 255.f ? 255.f : res);
            const unsigned byte = (unsigned)(int)res;
            if (full) res4 |= byte << (8 * k); else o[k] = (uint8_t)byte;
        }
        if (full) { UD u; u.v = res4; *reinterpret_cast<UD*>(o) = u; }
    }
}
void launch_clahe(const ClaheArgs& a, int n_seq, hipStream_t st) {
    const dim3 gl(a.tiles_x * a.tiles_y, a.ncam, n_seq), ga((a.th + 5 + CLAHE_ROWS - 1) / CLAHE_ROWS, a.tiles_y + 1, a.ncam * n_seq);
    const auto go = [&](auto b) {
        constexpr int BPP = decltype(b)::value;
        hipLaunchKernelGGL(k_clahe_lut<BPP>, gl, dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_clahe_apply<BPP>, ga, dim3(256), 0, st, a);
    };
    if (a.g.bpp <= 1) go(std::integral_constant<int, 1>{}); else with_bpp(a.g.bpp, go);
}

// svo_rectify_image: one thread per output pixel (all channels), packed output rows
template <int CN>
__global__ __launch_bounds__(256) void k_rectify_image(const short2* __restrict__ m1, const uint16_t* __restrict__ m2, int w, int h,
                                                       const uint8_t* __restrict__ raw, int rw, int rh, int stride, uint8_t* __restrict__ out) {
    const int total = w * h;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        uint8_t px[CN];
        remap_px<CN>(raw, stride, rw, rh, m1[i], m2[i], px);
#pragma unroll
        for (int c = 0; c < CN; c++) out[(size_t)i * CN + c] = px[c];
    }
}
void launch_rectify_image(const short2* map1, const uint16_t* map2, int w, int h, const uint8_t* raw, int raw_w, int raw_h, int raw_stride,
                          int cn, uint8_t* out, hipStream_t st) {
    int gx = (w * h + 255) / 256; if (gx > 4096) gx = 4096;
    if (cn == 3) hipLaunchKernelGGL(k_rectify_image<3>, dim3(gx), dim3(256), 0, st, map1, map2, w, h, raw, raw_w, raw_h, raw_stride, out);
    else hipLaunchKernelGGL(k_rectify_image<1>, dim3(gx), dim3(256), 0, st, map1, map2, w, h, raw, raw_w, raw_h, raw_stride, out);
}

// ------------------------------------------------------------------------------------------------
// frame begin / end: the slot bookkeeping of stereo_callback (vo.cpp:47-56, 74-75) and of the
// pyramid cache in circularMatching (vo.cpp:179-181 vs 231-232: the cache is NOT refreshed when
// there were no points to match — the "stale pyramid" quirk).
// ------------------------------------------------------------------------------------------------
// The per-frame reset with t1 as the frame's T1 slot: run once per sequence, by a thread of the ingest kernel (PYR_BEGIN) or by
// k_frame_begin.  (The bucket keys need no clearing: every detection pass leaves them zero, see k_bucket_emit.)
__device__ __forceinline__ void frame_begin(SeqState& s, int t1) {
    s.n_old = s.n_feat;
    s.active = s.frame_id > 0;
    s.slot_t1 = t1;
    s.do_second = 0; s.n_lk = 0; s.n_tracks = 0; s.n_circ = 0; s.n_inliers = 0; s.ok = 0;
    s.pnp_best = -1; s.pnp_iters = 0; s.pnp_good = 0; s.pnp_drawn = 0;
    s.fail_reason = s.active ? 0 : 1;
    svo_frame_stats z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    s.stats = z;
}
// The slot an ingest block writes.  PYR_BEGIN: the thread for which `first` holds (one per sequence: camera 0, block (0, 0),
// thread 0) also runs the reset; the other blocks need not wait for it, pyr_slot() reads no field the reset writes.
__device__ __forceinline__ int ingest_slot(const DevBuffers& d, int seq, PyrTarget target, bool first) {
    const int slot = pyr_slot(d.st[seq], target);
    if (target == PYR_BEGIN && first) frame_begin(d.st[seq], slot);
    return slot;
}

// One thread per sequence of the context, idle ones included: an idle sequence (ragged frame, d.act[B + seq] == 0) gets the row
// of a frame it did not take — its last good transform, ok 0, zero counters, fail_reason 5 — and nothing of its state is written.
__global__ void k_frame_end(DevBuffers d, int ring_slot) {
    int seq = blockIdx.x * blockDim.x + threadIdx.x;
    if (seq >= d.B) return;
    SeqState& s = d.st[seq];
    if (d.act && !d.act[d.B + seq]) {
        FrameResult& r = d.results[(size_t)ring_slot * d.B + seq];
        for (int i = 0; i < 16; i++) r.T[i] = s.last_T[i];
        r.ok = 0;
        svo_frame_stats z = {0, 0, 0, 0, 0, 0, 0, 5, 0, 0, 0};
        r.stats = z;
        return;
    }
    s.slot_img_t0 = s.slot_t1;                                   // vo.cpp:48-49 / 74-75
    if (!s.active || s.n_lk > 0) s.slot_pyr_t0 = s.slot_t1;      // vo.cpp:50-53 / 231-232 (skipped on the early return :179-181)
    s.frame_id++;
    FrameResult& r = d.results[(size_t)ring_slot * d.B + seq];
    for (int i = 0; i < 16; i++) r.T[i] = s.last_T[i];           // fail_result = last_transform (vo.cpp:43-44); on success last_T was just updated
    r.ok = s.ok;
    s.stats.fail_reason = s.fail_reason;
    s.stats.n_features_out = s.n_feat;
    s.stats.n_into_lk = s.n_lk;
    s.stats.n_after_circular = s.n_circ;
    s.stats.n_after_bounds = s.n_tracks;
    s.stats.n_inliers = s.n_inliers;
    s.stats.ransac_iters = s.pnp_iters;
    r.stats = s.stats;
}

void launch_frame_end(const DevBuffers& d, int ring_slot, hipStream_t st) {
    hipLaunchKernelGGL(k_frame_end, dim3((d.B + 63) / 64), dim3(64), 0, st, d, ring_slot);
}

// ------------------------------------------------------------------------------------------------
// ingest: the caller's two images into level 0 of the target's pyramid slot (the deep copies of vo.cpp:74-75 / the level-0 copy of
// cv::buildOpticalFlowPyramid), one thread per pixel.  CN = 3: interleaved BGR rows -> three planes (level 0 of the three
// per-plane pyramids).  RECT (rectifying contexts, d.rmap set): a pixel is the remap of the raw frame at the map's position
// instead of the caller's bytes.  Colour contexts also keep, for the left camera, the W x H byte image made of the first W bytes
// of every interleaved row — of every RECTIFIED interleaved row when rectifying — which is what cv::FAST scans in a 3-channel Mat
// (the reference quirk of svo.h, channels): bytes 3x .. 3x + 2 of that row are pixel x's three channels, so the threads of
// pixels x < W / 3 write them.
// ------------------------------------------------------------------------------------------------
template <int CN, bool RECT>
__global__ __launch_bounds__(256) void k_ingest(DevBuffers d, const uint8_t* const* srcs, int stride, PyrTarget target) {
    const int seq = seq_of(d, blockIdx.z), cam = blockIdx.y;
    const int W = d.geom.W, H = d.geom.H;
    const int total = W * H;
    const uint8_t* src = srcs[cam * d.B + seq];
    const int slot = ingest_slot(d, seq, target, blockIdx.x == 0 && cam == 0 && threadIdx.x == 0);
    uint8_t* p0 = d.pyr + pyr_index(d, seq, slot, cam) + d.geom.lv[0].off;
    const int dstride = d.geom.lv[0].stride;
    uint8_t* fi = CN == 3 ? d.fastimg + fastimg_index(d, seq, slot) : nullptr;
    const size_t pb = (size_t)d.geom.pyr_bytes;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int y = i / W, x = i - y * W;
        uint8_t px[CN];
        if constexpr (RECT) remap_px<CN>(src, stride, d.raw_w, d.raw_h, rect_map1(d, cam, seq)[i], rect_map2(d, cam, seq)[i], px);
        else {
#pragma unroll
            for (int c = 0; c < CN; c++) px[c] = src[(size_t)y * stride + CN * x + c];
        }
        const size_t o = (size_t)y * dstride + x;
#pragma unroll
        for (int c = 0; c < CN; c++) p0[c * pb + o] = px[c];
        if (CN == 3 && cam == 0) {
#pragma unroll
            for (int c = 0; c < CN; c++) if (3 * x + c < W) fi[(size_t)y * W + 3 * x + c] = px[c];
        }
    }
}
template <int CN, bool RECT>
static void launch_ingest_as(const DevBuffers& d, const uint8_t* const* ptrs, int stride, PyrTarget target, hipStream_t st) {
    int gx = (d.geom.W * d.geom.H + 255) / 256; if (gx > 2048) gx = 2048;
    hipLaunchKernelGGL((k_ingest<CN, RECT>), dim3(gx, 2, launch_seqs(d)), dim3(256), 0, st, d, ptrs, stride, target);
}
// k_ingest<1, RECT> of a converting context (d.in.bpp = BPP): a pixel is the grey value of the caller's pixel, or the remap of the
// grey raw frame
template <int BPP, bool RECT>
__global__ __launch_bounds__(256) void k_ingest_grey(DevBuffers d, const uint8_t* const* srcs, int stride, PyrTarget target) {
    const int seq = seq_of(d, blockIdx.z), cam = blockIdx.y;
    const int W = d.geom.W, H = d.geom.H;
    const int total = W * H;
    const uint8_t* src = srcs[cam * d.B + seq];
    const int slot = ingest_slot(d, seq, target, blockIdx.x == 0 && cam == 0 && threadIdx.x == 0);
    uint8_t* p0 = d.pyr + pyr_index(d, seq, slot, cam) + d.geom.lv[0].off;
    const int dstride = d.geom.lv[0].stride;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int y = i / W, x = i - y * W;
        uint8_t px;
        if constexpr (RECT) remap_grey_px<BPP>(src, stride, d.raw_w, d.raw_h, rect_map1(d, cam, seq)[i], rect_map2(d, cam, seq)[i], d.in, &px);
        else px = (uint8_t)grey_px<BPP>(src + (size_t)y * stride + (size_t)x * BPP, d.in);
        p0[(size_t)y * dstride + x] = px;
    }
}
static void launch_ingest(const DevBuffers& d, const uint8_t* const* ptrs, int stride, PyrTarget target, hipStream_t st) {
    if (d.CN == 1 && d.in.bpp > 1) {
        int gx = (d.geom.W * d.geom.H + 255) / 256; if (gx > 2048) gx = 2048;
        with_bpp(d.in.bpp, [&](auto b) {
            constexpr int BPP = decltype(b)::value;
            const auto k = d.rmap ? k_ingest_grey<BPP, true> : k_ingest_grey<BPP, false>;
            hipLaunchKernelGGL(k, dim3(gx, 2, launch_seqs(d)), dim3(256), 0, st, d, ptrs, stride, target);
        });
        return;
    }
    if (d.CN == 3) { if (d.rmap) launch_ingest_as<3, true>(d, ptrs, stride, target, st); else launch_ingest_as<3, false>(d, ptrs, stride, target, st); }
    else { if (d.rmap) launch_ingest_as<1, true>(d, ptrs, stride, target, st); else launch_ingest_as<1, false>(d, ptrs, stride, target, st); }
}

// ------------------------------------------------------------------------------------------------
// pyrDown (the level loop of cv::buildOpticalFlowPyramid, vo.cpp:50,52,200,201):
// dst(x,y) = (sum_{i,j} k_i k_j src(2x+i-2, 2y+j-2) + 128) >> 8, k = [1 4 6 4 1], REFLECT_101.
// A 256-thread block owns a TW x TH output tile: the (2 TW + 3) x (2 TH + 3) source tile staged in LDS, separable in two LDS
// passes.  The pieces below are shared by every pyrDown kernel; the LDS arrays are declared by the kernel bodies (k_front_a and
// k_front_b run one of them beside a detection body in one launch) and passed in.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned tap5(unsigned a, unsigned b, unsigned c, unsigned d, unsigned e) { return c * 6 + (b + d) * 4 + a + e; }
__device__ __forceinline__ unsigned pd_round(unsigned v) { return (v + 128) >> 8; }   // v = a sum of 25 products: <= 256 * 255

// The SW x SH source tile whose first pixel is (sx0, sy0) of a w x h level.  A tile whose padded rows (TS bytes: whole dwords) lie
// inside the level — almost all of them — is TS / 4 unaligned dword loads per row, no border arithmetic; any other one takes
// reflected bytes, and its columns SW .. TS - 1 stay unwritten (read by the paired pass below, never used).
template <int SW, int SH, int TS>
__device__ __forceinline__ void pd_fill_tile(uint8_t (&tile)[SH][TS], const uint8_t* src, int stride, int w, int h, int sx0, int sy0) {
    static_assert(TS % 4 == 0 && TS > SW, "tile rows are whole dwords");
    if (sx0 >= 0 && sy0 >= 0 && sx0 + TS <= w && sy0 + SH <= h) {
        constexpr int DPR = TS / 4;
        for (int i = threadIdx.x; i < DPR * SH; i += 256) {
            const int ty = i / DPR, c = i - ty * DPR;
            *reinterpret_cast<unsigned*>(&tile[ty][4 * c]) = reinterpret_cast<const UD*>(src + (size_t)(sy0 + ty) * stride + sx0 + 4 * c)->v;
        }
    } else {
        for (int i = threadIdx.x; i < SW * SH; i += 256) {
            const int ty = i / SW, tx = i - ty * SW;
            tile[ty][tx] = src[(size_t)reflect101(sy0 + ty, h) * stride + reflect101(sx0 + tx, w)];
        }
    }
}
// pd_fill_tile of a caller image in the format g (BPP bytes per pixel): the tile holds grey bytes.  Interior tiles: four pixels per
// thread, one LDS dword out (grey4: every byte it loads belongs to pixels sx0 .. sx0 + TS - 1 < w of the row); any other tile:
// the reflected pixel, converted.
template <int SW, int BPP, int SH, int TS>
__device__ __forceinline__ void grey_fill_tile(uint8_t (&tile)[SH][TS], const uint8_t* src, int stride, int w, int h, int sx0, int sy0, const GreyIn& g) {
    static_assert(TS % 4 == 0 && TS > SW, "tile rows are whole dwords");
    if (sx0 >= 0 && sy0 >= 0 && sx0 + TS <= w && sy0 + SH <= h) {
        constexpr int DPR = TS / 4;
        for (int i = threadIdx.x; i < DPR * SH; i += 256) {
            const int ty = i / DPR, c = i - ty * DPR;
            *reinterpret_cast<unsigned*>(&tile[ty][4 * c]) = grey4<BPP>(src + (size_t)(sy0 + ty) * stride + (size_t)(sx0 + 4 * c) * BPP, g);
        }
    } else {
        for (int i = threadIdx.x; i < SW * SH; i += 256) {
            const int ty = i / SW, tx = i - ty * SW;
            tile[ty][tx] = (uint8_t)grey_px<BPP>(src + (size_t)reflect101(sy0 + ty, h) * stride + (size_t)reflect101(sx0 + tx, w) * BPP, g);
        }
    }
}
// horizontal 1-4-6-4-1 pass, TWO outputs per thread (even TW): outputs 2j and 2j + 1 of a row read tile bytes 4j .. 4j + 6 = two
// aligned LDS dwords, and leave as one dword of hrow (a sum is <= 16 * 255)
template <int TW, int SH, int TS>
__device__ __forceinline__ void pd_hpass2(const uint8_t (&tile)[SH][TS], unsigned short (&hrow)[SH][TW]) {
    static_assert(TW % 2 == 0 && TS >= 2 * TW + 4, "rows of whole dwords");
    for (int i = threadIdx.x; i < SH * (TW / 2); i += 256) {
        const int ty = i / (TW / 2), j = i - ty * (TW / 2);
        const unsigned a = *reinterpret_cast<const unsigned*>(&tile[ty][4 * j]), b = *reinterpret_cast<const unsigned*>(&tile[ty][4 * j + 4]);
        const unsigned r0 = a & 255u, r1 = (a >> 8) & 255u, r2 = (a >> 16) & 255u, r3 = a >> 24, r4 = b & 255u, r5 = (b >> 8) & 255u, r6 = (b >> 16) & 255u;
        *reinterpret_cast<unsigned*>(&hrow[ty][2 * j]) = tap5(r0, r1, r2, r3, r4) | (tap5(r2, r3, r4, r5, r6) << 16);
    }
}
// vertical pass and rounding store of the TW x (SH - 3) / 2 outputs at (ox, oy) of level ld, two per thread: five LDS dwords, one
// 2-byte store
template <int TW, int SH>
__device__ __forceinline__ void pd_vpass2(const unsigned short (&hrow)[SH][TW], uint8_t* dst, const LevelInfo& ld, int ox, int oy) {
    constexpr int TH = (SH - 3) / 2;
    for (int i = threadIdx.x; i < TH * (TW / 2); i += 256) {
        const int y = i / (TW / 2), x = 2 * (i - y * (TW / 2));
        const int gx = ox + x, gy = oy + y;
        if (gx < ld.w && gy < ld.h) {
            unsigned q[5];
#pragma unroll
            for (int k = 0; k < 5; k++) q[k] = *reinterpret_cast<const unsigned*>(&hrow[2 * y + k][x]);
            const unsigned b0 = pd_round(tap5(q[0] & 0xFFFFu, q[1] & 0xFFFFu, q[2] & 0xFFFFu, q[3] & 0xFFFFu, q[4] & 0xFFFFu));
            const unsigned b1 = pd_round(tap5(q[0] >> 16, q[1] >> 16, q[2] >> 16, q[3] >> 16, q[4] >> 16));
            uint8_t* o = dst + (size_t)gy * ld.stride + gx;
            if (gx + 1 < ld.w) *reinterpret_cast<unsigned short*>(o) = (unsigned short)(b0 | (b1 << 8));   // gx is even, rows are 16-byte aligned
            else o[0] = (uint8_t)b0;
        }
    }
}

// k_pyrdown: one level from the one below it, 32 x 8 outputs per block (an odd last level, colour contexts, the stage calls)
#define PD_TW 32
#define PD_TH 8
__global__ __launch_bounds__(256) void k_pyrdown(DevBuffers d, int level, PyrTarget target) {
    const int plane = blockIdx.z % d.CN, sc = blockIdx.z / d.CN;          // every colour plane is its own pyramid
    const int seq = seq_of(d, sc / 2), cam = sc & 1;
    const LevelInfo ls = d.geom.lv[level - 1], ld = d.geom.lv[level];
    uint8_t* base = d.pyr + pyr_index(d, seq, pyr_slot(d.st[seq], target), cam) + (size_t)plane * d.geom.pyr_bytes;
    constexpr int SW = 2 * PD_TW + 3, SH = 2 * PD_TH + 3;        // 67 x 19 source tile
    __shared__ __attribute__((aligned(4))) uint8_t tile[SH][SW + 1];
    __shared__ __attribute__((aligned(4))) unsigned short hrow[SH][PD_TW];
    const int ox = blockIdx.x * PD_TW, oy = blockIdx.y * PD_TH;
    pd_fill_tile<SW>(tile, base + ls.off, ls.stride, ls.w, ls.h, 2 * ox - 2, 2 * oy - 2);
    __syncthreads();
    pd_hpass2<PD_TW>(tile, hrow);
    __syncthreads();
    pd_vpass2<PD_TW>(hrow, base + ld.off, ld, ox, oy);
}

// ---- fewer launches for the front of a frame (a lone stream is launch-bound there: a 5 us kernel every 4.5 us of host time) ----
// k_ingest_pyr1: ingest and the first pyrDown in one launch (single-channel contexts) = k_pyrdown's steps with the caller's image
// as the source and one more: the block also writes the 2 TW x 2 TH level-0 pixels it owns, from the tile.
// (bodies take their block coordinates as arguments so that k_front_a / k_front_b below can run two of them in one launch)
// TW x TH = the block's tile of level 1.  Lone streams: 32 x 8 (many blocks for one image).  Many-sequence contexts: 64 x 16 — at
// a thousand images per launch the kernel was bound by block turnover (962 000 blocks of 1 KB of output each: 0.68 ms per 512
// sequences = 1.6 TB/s), not by LDS or HBM; four times the work per block and half the halo.
// RECT (rectifying contexts, d.rmap set): the source tile is filled by remapping the raw frame — tile byte (tx, ty) = the rectified
// pixel at (reflect101(sx0 + tx), reflect101(sy0 + ty)), the byte the plain form reads from a rectified caller image — and the
// level-0 store and both pyrDown passes run unchanged on it.  The rectified level 0 never makes a round trip through memory.
// BPP > 1 (converting contexts, d.in.bpp = BPP): only the tile fill differs — it converts the caller's pixels (the four raw taps of
// a rectifying one) to grey on the way in; the tile holds grey bytes, and everything after the fill is the same code.
template <int TW, int TH, bool RECT, int BPP = 1>
static __device__ __forceinline__ void ingest_pyr1_body(const DevBuffers& d, const uint8_t* const* srcs, int stride, PyrTarget target, int bx, int by, int bz) {
    const int seq = seq_of(d, bz >> 1), cam = bz & 1;
    const LevelInfo ls = d.geom.lv[0], ld = d.geom.lv[1];
    const uint8_t* src = srcs[cam * d.B + seq];
    uint8_t* base = d.pyr + pyr_index(d, seq, ingest_slot(d, seq, target, bx == 0 && by == 0 && cam == 0 && threadIdx.x == 0), cam);
    uint8_t* l0 = base + ls.off;
    constexpr int SW = 2 * TW + 3, SH = 2 * TH + 3;              // 67 x 19 source tile at 32 x 8
    __shared__ __attribute__((aligned(4))) uint8_t tile[SH][SW + 1];
    __shared__ __attribute__((aligned(4))) unsigned short hrow[SH][TW];
    const int ox = bx * TW, oy = by * TH;
    const int sx0 = 2 * ox - 2, sy0 = 2 * oy - 2;
    if constexpr (RECT) {
        const short2* m1 = rect_map1(d, cam, seq); const uint16_t* m2 = rect_map2(d, cam, seq);
        for (int i = threadIdx.x; i < SW * SH; i += 256) {
            const int ty = i / SW, tx = i - ty * SW;
            const int m = reflect101(sy0 + ty, ls.h) * ls.w + reflect101(sx0 + tx, ls.w);
            if constexpr (BPP == 1) remap_px<1>(src, stride, d.raw_w, d.raw_h, m1[m], m2[m], &tile[ty][tx]);
            else remap_grey_px<BPP>(src, stride, d.raw_w, d.raw_h, m1[m], m2[m], d.in, &tile[ty][tx]);
        }
    } else if constexpr (BPP == 1) pd_fill_tile<SW>(tile, src, stride, ls.w, ls.h, sx0, sy0);
    else grey_fill_tile<SW, BPP>(tile, src, stride, ls.w, ls.h, sx0, sy0, d.in);
    __syncthreads();
    // the block's own 2 TW x 2 TH level-0 pixels: in range, so the tile holds the pixels themselves
    if (2 * ox + 2 * TW <= ls.w && 2 * oy + 2 * TH <= ls.h) {     // all inside the level: a dword at a time (tile bytes 4c + 2 .. 4c + 5: two aligned LDS dwords, shifted)
        for (int i = threadIdx.x; i < (TW / 2) * (2 * TH); i += 256) {
            const int ty = i / (TW / 2), c = i - ty * (TW / 2);
            const unsigned lo = *reinterpret_cast<const unsigned*>(&tile[ty + 2][4 * c]), hi = *reinterpret_cast<const unsigned*>(&tile[ty + 2][4 * c + 4]);
            UD u; u.v = __builtin_amdgcn_alignbyte(hi, lo, 2);
            *reinterpret_cast<UD*>(l0 + (size_t)(2 * oy + ty) * ls.stride + 2 * ox + 4 * c) = u;
        }
    } else {
        for (int i = threadIdx.x; i < 2 * TW * 2 * TH; i += 256) {
            const int ty = i / (2 * TW), tx = i - ty * (2 * TW);
            const int gx = 2 * ox + tx, gy = 2 * oy + ty;
            if (gx < ls.w && gy < ls.h) l0[(size_t)gy * ls.stride + gx] = tile[ty + 2][tx + 2];
        }
    }
    pd_hpass2<TW>(tile, hrow);
    __syncthreads();
    pd_vpass2<TW>(hrow, base + ld.off, ld, ox, oy);
}
#define IG_TW 64
#define IG_TH 16
template <int TW, int TH, bool RECT>
__global__ __launch_bounds__(256) void k_ingest_pyr1(DevBuffers d, const uint8_t* const* srcs, int stride, PyrTarget target) {
    ingest_pyr1_body<TW, TH, RECT>(d, srcs, stride, target, blockIdx.x, blockIdx.y, blockIdx.z);
}
template <int TW, int TH, bool RECT>
static void launch_ingest_pyr1_as(const DevBuffers& d, const uint8_t* const* ptrs, int stride, PyrTarget target, hipStream_t st) {
    dim3 g((d.geom.lv[1].w + TW - 1) / TW, (d.geom.lv[1].h + TH - 1) / TH, launch_seqs(d) * 2);
    hipLaunchKernelGGL((k_ingest_pyr1<TW, TH, RECT>), g, dim3(256), 0, st, d, ptrs, stride, target);
}
// the converting forms: symbols of their own beside k_ingest_pyr1 (whose instantiations stay what they were), the same body
template <int BPP, int TW, int TH, bool RECT>
__global__ __launch_bounds__(256) void k_ingest_pyr1_grey(DevBuffers d, const uint8_t* const* srcs, int stride, PyrTarget target) {
    ingest_pyr1_body<TW, TH, RECT, BPP>(d, srcs, stride, target, blockIdx.x, blockIdx.y, blockIdx.z);
}
template <int BPP, int TW, int TH>
static void launch_ingest_pyr1_grey_as(const DevBuffers& d, const uint8_t* const* ptrs, int stride, PyrTarget target, hipStream_t st) {
    dim3 g((d.geom.lv[1].w + TW - 1) / TW, (d.geom.lv[1].h + TH - 1) / TH, launch_seqs(d) * 2);
    const auto k = d.rmap ? k_ingest_pyr1_grey<BPP, TW, TH, true> : k_ingest_pyr1_grey<BPP, TW, TH, false>;
    hipLaunchKernelGGL(k, g, dim3(256), 0, st, d, ptrs, stride, target);
}
static void launch_ingest_pyr1(const DevBuffers& d, const uint8_t* const* ptrs, int stride, PyrTarget target, hipStream_t st) {
    if (d.in.bpp > 1) {
        with_bpp(d.in.bpp, [&](auto b) {
            constexpr int BPP = decltype(b)::value;
            if (d.B > SVO_LONE_MAX_SEQ) launch_ingest_pyr1_grey_as<BPP, IG_TW, IG_TH>(d, ptrs, stride, target, st);
            else launch_ingest_pyr1_grey_as<BPP, PD_TW, PD_TH>(d, ptrs, stride, target, st);
        });
        return;
    }
    if (d.B > SVO_LONE_MAX_SEQ) { if (d.rmap) launch_ingest_pyr1_as<IG_TW, IG_TH, true>(d, ptrs, stride, target, st); else launch_ingest_pyr1_as<IG_TW, IG_TH, false>(d, ptrs, stride, target, st); }
    else { if (d.rmap) launch_ingest_pyr1_as<PD_TW, PD_TH, true>(d, ptrs, stride, target, st); else launch_ingest_pyr1_as<PD_TW, PD_TH, false>(d, ptrs, stride, target, st); }
}

// k_pyrdown2: levels l+1 AND l+2 from level l in one launch.  A block owns a 16 x 8 tile of level l+2, i.e. 32 x 16 of level l+1;
// it computes the 35 x 19 level-(l+1) pixels its own tile needs (the 3-pixel rim is recomputed by the neighbours: +30 % work on
// levels that are 1/16 and 1/64 of the image) from a 73 x 41 source tile.  Rim positions outside level l+1 are never read:
// REFLECT_101 folds them onto positions inside the tile.  (The middle tile is 35 wide — odd — so the passes go an output at a time.)
#define P2_TW 16
#define P2_TH 8
static __device__ __forceinline__ void pyrdown2_body(const DevBuffers& d, int level, PyrTarget target, int bx, int by, int bz) {
    const int plane = bz % d.CN, sc = bz / d.CN;
    const int seq = seq_of(d, sc / 2), cam = sc & 1;
    const LevelInfo ls = d.geom.lv[level], lm = d.geom.lv[level + 1], ld = d.geom.lv[level + 2];
    uint8_t* base = d.pyr + pyr_index(d, seq, pyr_slot(d.st[seq], target), cam) + (size_t)plane * d.geom.pyr_bytes;
    uint8_t* mid = base + lm.off; uint8_t* dst = base + ld.off;
    constexpr int MW = 2 * P2_TW + 3, MH = 2 * P2_TH + 3;        // 35 x 19 of the middle level
    constexpr int SW = 2 * MW + 3, SH = 2 * MH + 3;              // 73 x 41 of the source level
    __shared__ __attribute__((aligned(4))) uint8_t tile[SH][SW + 3];
    __shared__ unsigned short hrow[SH][MW + 1];
    __shared__ uint8_t mtile[MH][MW + 1];
    __shared__ unsigned short hrow2[MH][P2_TW];
    const int ox = bx * P2_TW, oy = by * P2_TH;                  // level l+2
    const int mx0 = 2 * ox - 2, my0 = 2 * oy - 2;                // level l+1
    pd_fill_tile<SW>(tile, base + ls.off, ls.stride, ls.w, ls.h, 2 * mx0 - 2, 2 * my0 - 2);
    __syncthreads();
    for (int i = threadIdx.x; i < SH * MW; i += 256) {
        const int ty = i / MW, x = i - ty * MW;
        const uint8_t* r = &tile[ty][2 * x];
        hrow[ty][x] = (unsigned short)tap5(r[0], r[1], r[2], r[3], r[4]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < MH * MW; i += 256) {
        const int y = i / MW, x = i - y * MW;
        const uint8_t m = (uint8_t)pd_round(tap5(hrow[2 * y][x], hrow[2 * y + 1][x], hrow[2 * y + 2][x], hrow[2 * y + 3][x], hrow[2 * y + 4][x]));
        mtile[y][x] = m;
        const int gx = mx0 + x, gy = my0 + y;
        if (x >= 2 && x < 2 + 2 * P2_TW && y >= 2 && y < 2 + 2 * P2_TH && gx < lm.w && gy < lm.h) mid[(size_t)gy * lm.stride + gx] = m;   // the owned 32 x 16
    }
    __syncthreads();
    for (int i = threadIdx.x; i < MH * P2_TW; i += 256) {
        const int ty = i / P2_TW, x = i - ty * P2_TW;
        // row / column of the middle tile that holds this (possibly folded) position; outputs beyond the level's edge (never
        // stored) may fold outside the tile: clamped, so that no index leaves the array
        int gy = reflect101(my0 + ty, lm.h) - my0;
        gy = gy < 0 ? 0 : gy > MH - 1 ? MH - 1 : gy;
        unsigned t[5];
#pragma unroll
        for (int k = 0; k < 5; k++) {
            int gx = reflect101(mx0 + 2 * x + k, lm.w) - mx0;
            gx = gx < 0 ? 0 : gx > MW - 1 ? MW - 1 : gx;
            t[k] = mtile[gy][gx];
        }
        hrow2[ty][x] = (unsigned short)tap5(t[0], t[1], t[2], t[3], t[4]);
    }
    __syncthreads();
    if (threadIdx.x < P2_TW * P2_TH) {
        const int y = threadIdx.x / P2_TW, x = threadIdx.x - y * P2_TW;
        const int gx = ox + x, gy = oy + y;
        if (gx < ld.w && gy < ld.h)
            dst[(size_t)gy * ld.stride + gx] = (uint8_t)pd_round(tap5(hrow2[2 * y][x], hrow2[2 * y + 1][x], hrow2[2 * y + 2][x], hrow2[2 * y + 3][x], hrow2[2 * y + 4][x]));
    }
}
__global__ __launch_bounds__(256) void k_pyrdown2(DevBuffers d, int level, PyrTarget target) { pyrdown2_body(d, level, target, blockIdx.x, blockIdx.y, blockIdx.z); }

// k_pyr_walk: one pyrDown level without LDS, for the plain many-sequence contexts (pyr_walk_applies).  A thread owns PW_VEC = 8
// consecutive outputs of a destination row — one aligned 8-byte store — and walks PW_ROWS rows down (svo_pyr_walk.hpp: the plan and
// the walk, which a host program runs too).  Per destination row it loads the 20 source bytes of two new source rows (from column
// 2 x0 - 2: the six aligned dwords around them, shifted into place — loading them as they lie, 16 unaligned bytes and a dword,
// measured the same), runs the horizontal 1-4-6-4-1 pass on 16-bit pairs (v_perm picks the taps of two outputs, v_pk_* sums them:
// <= 16 * 255) and adds the row into two running column sums instead of keeping five rows: with e = row 2y + 2 and o = row 2y + 1,
//   out(y) = (A + 4 o + e + 128) >> 8,   A' = B + 4 o + 6 e,   B' = e            (A = rows 2y-2, 2y-1, 2y weighted 1 4 6; B = row 2y)
// — the same integers as the five-tap sum (<= 256 * 255 + 128: they fit the 16-bit lanes), eight registers of state.
// Source rows outside the level are the reflected rows (a row offset, no other cost).  The first vector of a row and the last one
// to three, whose loads would leave the row, take the edge form: every dword from the nearest place inside the row, its bytes
// folded into place by one v_perm — as cheap as the fast form, which matters: a first version that fetched their reflected bytes
// one by one took 780 us per 512 sequences where this one takes 420.
// INGEST: the source is the caller's image (k_ingest_pyr1's job): the thread also stores the level-0 bytes 2 x0 .. 2 x0 + 15 of
// every source row it is the first to load (rows 2y + 1 and 2y + 2 of its destination rows, row 0 in the first group) from the
// dwords it holds — 16 bytes at a 4-byte aligned address — and the launch runs the reset duty of ingest_slot.  It walks 16 rows
// (8 measured 498 us, 16 419 us; the levels >= 2 are as fast with 8).  No byte outside the h rows of w bytes of the caller's image
// is ever loaded, whatever its stride or alignment: svo_pyr_walk.hpp's plan, checked on the host (tests/test_pyr_walk_cases.py).
template <bool INGEST>
__global__ __launch_bounds__(256) void k_pyr_walk(DevBuffers d, const uint8_t* const* srcs, int stride, int level, PyrTarget target) {
    const int seq = seq_of(d, blockIdx.z), cam = blockIdx.y;
    const int slot = INGEST ? ingest_slot(d, seq, target, blockIdx.x == 0 && cam == 0 && threadIdx.x == 0) : pyr_slot(d.st[seq], target);
    const LevelInfo ls = d.geom.lv[level - 1], ld = d.geom.lv[level];
    const PwPlan p = pw_plan(ls.w, ls.h, d.geom.pad, INGEST ? PW_ROWS_INGEST : PW_ROWS);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pw_items(p)) return;
    const PwItem it = pw_item(p, i);
    uint8_t* base = d.pyr + pyr_index(d, seq, slot, cam);
    const uint8_t* src = INGEST ? srcs[cam * d.B + seq] : base + ls.off;
    const int ss = INGEST ? stride : ls.stride, rows = pw_item_rows(p, it);
    if (it.mode == PW_FAST) pw_walk<INGEST, PW_FAST>(src, ss, ls.w, ls.h, base + ls.off, ls.stride, base + ld.off, ld.stride, ld.w, it.x0, it.y0, rows);
    else if (it.mode == PW_EDGE) pw_walk<INGEST, PW_EDGE>(src, ss, ls.w, ls.h, base + ls.off, ls.stride, base + ld.off, ld.stride, ld.w, it.x0, it.y0, rows);
    else pw_walk<INGEST, PW_TINY>(src, ss, ls.w, ls.h, base + ls.off, ls.stride, base + ld.off, ld.stride, ld.w, it.x0, it.y0, rows);
}
// SVO_PYR_WALK=0 (read once per process) keeps the LDS-tiled kernels for these contexts too: the A/B switch
static bool pyr_walk_applies(const DevBuffers& d) {
    static const bool off = getenv("SVO_PYR_WALK") && atoi(getenv("SVO_PYR_WALK")) == 0;
    return !off && d.B > SVO_LONE_MAX_SEQ && d.CN == 1 && d.in.bpp <= 1 && !d.rmap;
}
template <bool INGEST>
static void launch_pyr_walk(const DevBuffers& d, const uint8_t* const* ptrs, int stride, int level, PyrTarget target, hipStream_t st) {
    const PwPlan p = pw_plan(d.geom.lv[level - 1].w, d.geom.lv[level - 1].h, d.geom.pad, INGEST ? PW_ROWS_INGEST : PW_ROWS);
    hipLaunchKernelGGL((k_pyr_walk<INGEST>), dim3((pw_items(p) + 255) / 256, 2, launch_seqs(d)), dim3(256), 0, st, d, ptrs, stride, level, target);
}

// k_pad_pyramid: the REFLECT_101 border of every level of the target's slot — what cv::buildOpticalFlowPyramid's copyMakeBorder leaves
// around each level (pyrBorder = BORDER_REFLECT_101).  Pixel (x, y) outside the level takes level(reflect101(y), reflect101(x)), the
// iterated borderInterpolate rule over the whole pad, also where the pad is wider than the level.  The border is written in DWORDS (row
// starts, the pad and pixel (0, 0) are 4-byte aligned): the ring of a level is cut into its top and bottom bands (pad rows of the
// padded width) and, per image row, the left band and the right band — the latter from the aligned x at or below the level's width,
// so up to three pixels of the level itself are rewritten with their own values.
// The four source bytes of a dword are consecutive ascending (one unaligned dword load) or descending (load + byte swap) except
// where a dword straddles a fold of a level narrower than the pad: those go byte by byte.  (First version: one thread, one byte
// load and one byte store per border pixel — 0.39 ms per 512 sequences; the image stream's kernels run in the gap between two LK
// launches, so their time is whole-job time.)
// (Second version: one thread per border DWORD of one flat list over all levels — 0.26 ms: two divisions and five folds per dword.)
// Now by rows.  The dwords written and their values are the same; what changed is who computes them:
// - top and bottom bands over the level's own columns: band row y there IS row reflect101(y) of the level, at the same alignment,
//   so a thread copies an aligned 16 bytes (columns xa + 16 c .. + 15, xa = the first 16-byte boundary at or behind pixel 0): one
//   division per 16 bytes and no fold but the row's;
// - everything left and right of that — the left and right bands of the image rows, and in the band rows the corners with the few
//   columns the 16-byte copies leave — PAD_LANES = 8 consecutive threads per row and side: they fold their row once and take the
//   side's dwords in turn (a band of 28 pixels is 7 or 8 dwords: one round; consecutive lanes store consecutive dwords).  A dword
//   whose four source bytes lie one fold out is one unaligned load and a byte swap, one inside the level an aligned load; only a
//   dword that straddles an edge or lies more than one fold out (levels narrower than the pad) folds byte by byte, as before.
// The grid walks ONE list of the work items of all levels (blockIdx.x, in level order; a block stays inside one level): the sides
// of all h + 2 pad rows first, then the copies — every block has a full share, whatever the size of its level.
#define PAD_LANES 4
__host__ __device__ inline int pad_xa(int P) { return (16 - (P & 15)) & 15; }
__host__ __device__ inline int pad_chunks(const LevelInfo& L, int P) { return L.w > pad_xa(P) ? (L.w - pad_xa(P)) >> 4 : 0; }
__host__ __device__ inline int pad_items(const LevelInfo& L, int P) { return 2 * PAD_LANES * (L.h + 2 * P) + 2 * P * pad_chunks(L, P); }
// the border dword at columns x .. x + 3 (x a multiple of 4, anywhere) of a row whose level pixels start at srow
__device__ __forceinline__ unsigned pad_dword(const uint8_t* __restrict__ srow, int x, int w) {
    if (x >= 0 && x + 3 < w) return *reinterpret_cast<const unsigned*>(srow + x);
    if (x + 3 < 0 && -x < w) return __builtin_bswap32(reinterpret_cast<const UD*>(srow - x - 3)->v);                 // columns -x, -x - 1, ..
    if (x >= w && 2 * w - 5 - x >= 0) return __builtin_bswap32(reinterpret_cast<const UD*>(srow + (2 * w - 5 - x))->v);   // 2 w - 2 - x, ..
    return (unsigned)srow[reflect101(x, w)] | ((unsigned)srow[reflect101(x + 1, w)] << 8) | ((unsigned)srow[reflect101(x + 2, w)] << 16) | ((unsigned)srow[reflect101(x + 3, w)] << 24);
}
__global__ __launch_bounds__(256) void k_pad_pyramid(DevBuffers d, PyrTarget target) {
    const int plane = blockIdx.z % d.CN, sc = blockIdx.z / d.CN;
    const int seq = seq_of(d, sc / 2), cam = sc & 1, P = d.geom.pad;
    int level = 0, blk = blockIdx.x;
    for (; level + 1 < d.geom.nlevels; level++) { const int n = (pad_items(d.geom.lv[level], P) + 255) >> 8; if (blk < n) break; blk -= n; }
    const LevelInfo L = d.geom.lv[level];
    const int w = L.w, h = L.h;
    uint8_t* img = d.pyr + pyr_index(d, seq, pyr_slot(d.st[seq], target), cam) + (size_t)plane * d.geom.pyr_bytes + L.off;
    const int nside = 2 * PAD_LANES * (h + 2 * P), nch = pad_chunks(L, P), xa = pad_xa(P), xb = xa + 16 * nch;
    const int i = blk * 256 + threadIdx.x;
    if (i < nside) {
        const int rs = i / PAD_LANES, y = (rs >> 1) - P;
        const bool right = rs & 1, band = y < 0 || y >= h;
        const uint8_t* srow = img + reflect101(y, h) * L.stride;
        uint8_t* drow = img + y * L.stride;
        const int xe = right ? P + ((w + 3) & ~3) : band ? xa : 0;       // the last dword of a row may reach into its stride padding
        for (int x = (right ? (band ? xb : w & ~3) : -P) + 4 * (i % PAD_LANES); x < xe; x += 4 * PAD_LANES) *reinterpret_cast<unsigned*>(drow + x) = pad_dword(srow, x, w);
    } else if (i < nside + 2 * P * nch) {
        const int j = i - nside, r = j / nch, x = xa + 16 * (j - r * nch), y = r < P ? r - P : h + r - P;
        *reinterpret_cast<uint4*>(img + y * L.stride + x) = *reinterpret_cast<const uint4*>(img + reflect101(y, h) * L.stride + x);
    }
}
static void launch_pad_pyramid(const DevBuffers& d, hipStream_t st, PyrTarget target) {
    int blocks = 0;
    for (int l = 0; l < d.geom.nlevels; l++) blocks += (pad_items(d.geom.lv[l], d.geom.pad) + 255) >> 8;
    hipLaunchKernelGGL(k_pad_pyramid, dim3(blocks, 1, launch_seqs(d) * 2 * d.CN), dim3(256), 0, st, d, target);
}

// k_deriv_levels: the Scharr images of the levels >= 1 of the target's slot, for the LK kernel (svo_internal.hpp: the derivative
// pyramid; contexts with d.deriv only).  Runs behind k_pad_pyramid: a sample inside the level is the derivative of the level WITH its
// REFLECT_101 border, at 4 x the Scharr value, the integers lk_pass computes for itself where there are no planes:
//   t0(c) = 12 (s[y-1][c] + s[y+1][c]) + 40 s[y][c]      t1(c) = s[y+1][c] - s[y-1][c]
//   Ix(x, y) = t0(x+1) - t0(x-1)                          Iy(x, y) = 12 (t1(x-1) + t1(x+1)) + 40 t1(x)        (|.| <= 16 320)
// One launch covers every level >= 1 (blockIdx.x walks their work items in level order, a block stays inside one level), both
// cameras and the launch's sequences.  No LDS: a thread owns DV_VEC = 8 consecutive samples of a row — one 16-byte store per plane —
// and walks DV_ROWS rows down with three source rows in registers, so a source row is loaded (DV_ROWS + 2) / DV_ROWS times.  The
// vectors start at x = 8 v - (pad & 7): pixel (0, 0) sits pad bytes behind a 16-byte boundary and pad is a multiple of 4, so that
// origin makes the 8-byte pixel load and both 16-byte stores aligned.  A source row is three aligned loads — the dword before the
// vector (its last byte is column x - 1), the vector's 8 bytes, the dword after it (its first byte is column x + 8; loaded only
// where a sample inside the level needs it) — which stay inside the stored border: bytes -8 .. w + 6 of rows -1 .. h (pad >= 8).
// Only samples inside the level are written: the planes' zero border stays as the allocation left it; the first and the last
// vector of a row, which may reach outside, store sample by sample.  (First version: a 64 x 16 LDS tile per block, four samples and
// 8 bytes per plane per thread.)
#define DV_VEC 8
#define DV_ROWS 8
__host__ __device__ inline int deriv_vectors(const LevelInfo& L, int pad) { return (L.w + (pad & 7) + DV_VEC - 1) / DV_VEC; }
__host__ __device__ inline int deriv_blocks(const LevelInfo& L, int pad) { return (deriv_vectors(L, pad) * ((L.h + DV_ROWS - 1) / DV_ROWS) + 255) / 256; }
// A source row in registers: columns 0 .. 11 of the vector (column c = pixel x - 1 + c; 0 .. 9 are used), and pair K = columns
// 2 K and 2 K + 1 as two 16-bit lanes — the arithmetic runs on such pairs (v_pk_*: every value fits 16 bits), and a pair of
// results is the dword that is stored.
typedef short dv_s2 __attribute__((ext_vector_type(2)));
struct DerivRow { unsigned s0, s1, s2; };
__device__ __forceinline__ DerivRow deriv_load_row(const uint8_t* __restrict__ p, bool right) {   // p: the vector's first pixel in that row
    const unsigned lo = *reinterpret_cast<const unsigned*>(p - 4);
    const uint2 m = *reinterpret_cast<const uint2*>(p);
    const unsigned hi = right ? *reinterpret_cast<const unsigned*>(p + 8) : 0u;
    return {__builtin_amdgcn_alignbyte(m.x, lo, 3), __builtin_amdgcn_alignbyte(m.y, m.x, 3), __builtin_amdgcn_alignbyte(hi, m.y, 3)};
}
template <int K>
__device__ __forceinline__ dv_s2 deriv_pair(const DerivRow& r) {
    const unsigned s = K < 2 ? r.s0 : K < 4 ? r.s1 : r.s2;
    return __builtin_bit_cast(dv_s2, __builtin_amdgcn_perm(s, s, (K & 1) ? 0x0c030c02u : 0x0c010c00u));
}
// pairs K - 1 of Ix and Iy of the row between a and c, from the column sums of pairs K - 1 (t0p, t1p) and K, which it leaves behind
template <int K>
__device__ __forceinline__ void deriv_step(const DerivRow& a, const DerivRow& b, const DerivRow& c, dv_s2& t0p, dv_s2& t1p, unsigned (&ix)[DV_VEC / 2], unsigned (&iy)[DV_VEC / 2]) {
    const dv_s2 pa = deriv_pair<K>(a), pb = deriv_pair<K>(b), pc = deriv_pair<K>(c);
    const dv_s2 t0 = (pa + pc) * (short)12 + pb * (short)40, t1 = pc - pa;
    if constexpr (K > 0) {
        ix[K - 1] = __builtin_bit_cast(unsigned, (dv_s2)(t0 - t0p));                 // columns 2 K, 2 K + 1 minus 2 K - 2, 2 K - 1
        const dv_s2 mid = __builtin_bit_cast(dv_s2, __builtin_amdgcn_alignbyte(__builtin_bit_cast(unsigned, t1), __builtin_bit_cast(unsigned, t1p), 2));   // columns 2 K - 1, 2 K
        iy[K - 1] = __builtin_bit_cast(unsigned, (dv_s2)((t1p + t1) * (short)12 + mid * (short)40));
    }
    t0p = t0; t1p = t1;
}
// the vector's samples of one row: 16 bytes where all eight lie inside the level, else the ones that do, one by one
__device__ __forceinline__ void deriv_store(int16_t* __restrict__ q, const unsigned (&v)[DV_VEC / 2], int x, int w) {
    if (x >= 0 && x + DV_VEC <= w) *reinterpret_cast<uint4*>(q) = make_uint4(v[0], v[1], v[2], v[3]);
    else {
#pragma unroll
        for (int j = 0; j < DV_VEC; j++) if ((unsigned)(x + j) < (unsigned)w) q[j] = (int16_t)(v[j >> 1] >> (16 * (j & 1)));
    }
}
__global__ __launch_bounds__(256) void k_deriv_levels(DevBuffers d, PyrTarget target) {
    const int P = d.geom.pad;
    int level = 1, b = blockIdx.x;
    for (; level + 1 < d.geom.nlevels; level++) { const int n = deriv_blocks(d.geom.lv[level], P); if (b < n) break; b -= n; }
    const LevelInfo L = d.geom.lv[level];
    const int w = L.w, h = L.h, nv = deriv_vectors(L, P);
    const int i = b * 256 + threadIdx.x, g = i / nv, x = (i - g * nv) * DV_VEC - (P & 7), y0 = g * DV_ROWS;
    if (y0 >= h) return;
    const int seq = seq_of(d, blockIdx.z), cam = blockIdx.y, slot = pyr_slot(d.st[seq], target);
    // one uniform base per array and 32-bit offsets beside it (a pyramid is far below 4 GB): two registers where three pointers took six
    const uint8_t* __restrict__ img = d.pyr + pyr_index(d, seq, slot, cam);
    int16_t* __restrict__ dx = d.deriv + deriv_index(d, seq, slot, cam);
    int16_t* __restrict__ dy = dx + deriv_samples(d.geom);
    unsigned io = (unsigned)(L.off + (y0 - 1) * L.stride + x), so = (unsigned)(L.off - deriv_origin(d.geom) + y0 * L.stride + x);
    const bool right = x + DV_VEC <= w;                              // column x + 8 is the neighbour of a sample inside the level
    const int rows = h - y0 < DV_ROWS ? h - y0 : DV_ROWS;
    DerivRow ra = deriv_load_row(img + io, right), rb = deriv_load_row(img + (io + L.stride), right);
    io += 2 * L.stride;
#pragma unroll 1
    for (int r = 0; r < rows; r++) {
        const DerivRow rc = deriv_load_row(img + io, right);
        unsigned ix[DV_VEC / 2], iy[DV_VEC / 2];
        dv_s2 t0p, t1p;
        deriv_step<0>(ra, rb, rc, t0p, t1p, ix, iy); deriv_step<1>(ra, rb, rc, t0p, t1p, ix, iy); deriv_step<2>(ra, rb, rc, t0p, t1p, ix, iy);
        deriv_step<3>(ra, rb, rc, t0p, t1p, ix, iy); deriv_step<4>(ra, rb, rc, t0p, t1p, ix, iy);
        deriv_store(dx + so, ix, x, w);
        deriv_store(dy + so, iy, x, w);
        ra = rb; rb = rc;
        io += L.stride; so += L.stride;
    }
}
static void launch_deriv_levels(const DevBuffers& d, hipStream_t st, PyrTarget target) {
    if (!d.deriv || d.geom.nlevels < 2) return;
    int blocks = 0;
    for (int l = 1; l < d.geom.nlevels; l++) blocks += deriv_blocks(d.geom.lv[l], d.geom.pad);
    hipLaunchKernelGGL(k_deriv_levels, dim3(blocks, 2, launch_seqs(d)), dim3(256), 0, st, d, target);
}

// levels first .. nlevels-1 from level first-1: pairs of levels per launch where two remain
static void launch_pyramid_from(const DevBuffers& d, int first, hipStream_t st, PyrTarget target) {
    if (pyr_walk_applies(d)) {                                       // level by level: one more small launch, no LDS
        for (int l = first; l < d.geom.nlevels; l++) launch_pyr_walk<false>(d, nullptr, 0, l, target, st);
        return;
    }
    int l = first;
    while (l < d.geom.nlevels) {
        if (l + 1 < d.geom.nlevels) {
            dim3 g((d.geom.lv[l + 1].w + P2_TW - 1) / P2_TW, (d.geom.lv[l + 1].h + P2_TH - 1) / P2_TH, launch_seqs(d) * 2 * d.CN);
            hipLaunchKernelGGL(k_pyrdown2, g, dim3(256), 0, st, d, l - 1, target);
            l += 2;
        } else {
            dim3 g((d.geom.lv[l].w + PD_TW - 1) / PD_TW, (d.geom.lv[l].h + PD_TH - 1) / PD_TH, launch_seqs(d) * 2 * d.CN);
            hipLaunchKernelGGL(k_pyrdown, g, dim3(256), 0, st, d, l, target);
            l += 1;
        }
    }
}
void launch_pyramid(const DevBuffers& d, hipStream_t st) { launch_pyramid_from(d, 1, st, PYR_T1); launch_pad_pyramid(d, st, PYR_T1); }

// ---- the next frame's pyramids, ahead of the frame (many-sequence contexts; svo_api.hip issue_frame) ----
// k_pick_next: one thread per sequence names the slot (a single decision per sequence: the blocks of the ingest that follows must
// all write the same one, whatever k_frame_end of the frame in flight does to the fields meanwhile).
__global__ void k_pick_next(DevBuffers d) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= launch_seqs(d)) return;
    const int seq = seq_of(d, b);
    d.st[seq].slot_next = next_slot(d.st[seq]);
}
__global__ void k_frame_begin(DevBuffers d) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= launch_seqs(d)) return;
    const int seq = seq_of(d, b);
    frame_begin(d.st[seq], d.st[seq].slot_next);
}
bool ingest_ahead_applies(const DevBuffers& d) {
    static const bool off = getenv("SVO_INGEST_AHEAD") && atoi(getenv("SVO_INGEST_AHEAD")) == 0;
    return !off && d.B > SVO_LONE_MAX_SEQ && d.CN == 1 && d.geom.nlevels >= 2;
}
void launch_frame_begin(const DevBuffers& d, hipStream_t st) {
    hipLaunchKernelGGL(k_frame_begin, dim3((launch_seqs(d) + 63) / 64), dim3(64), 0, st, d);
}

// ingest + all pyramid levels + their borders into the target's slot (vo.cpp:74-75, 200-201): single-channel contexts fuse the
// ingest with the first level.  A PYR_BEGIN ingest runs the reset, which names its slot T1: that is what the kernels after it build on.
void launch_ingest_pyramid(const DevBuffers& d, const uint8_t* const* left_right_dev_ptrs, int stride, hipStream_t st, PyrTarget target) {
    if (target == PYR_NEXT) hipLaunchKernelGGL(k_pick_next, dim3((launch_seqs(d) + 63) / 64), dim3(64), 0, st, d);
    const PyrTarget rest = target == PYR_BEGIN ? PYR_T1 : target;
    if (d.CN == 1 && d.geom.nlevels >= 2) {
        if (pyr_walk_applies(d)) launch_pyr_walk<true>(d, left_right_dev_ptrs, stride, 1, target, st);
        else launch_ingest_pyr1(d, left_right_dev_ptrs, stride, target, st);
        launch_pyramid_from(d, 2, st, rest);
    } else {
        launch_ingest(d, left_right_dev_ptrs, stride, target, st);
        launch_pyramid_from(d, 1, st, rest);
    }
    launch_pad_pyramid(d, st, rest);
    launch_deriv_levels(d, st, rest);                                // contexts with a derivative pyramid: every pyramid they build gets its planes
}

// svo_reset_sequence: the fields the constructor sets (vo.h:266-268, svo_api.hip ctx_create) and nothing else — frame_id = 0 makes
// the next frame a first frame, whose reset picks its T1 slot afresh.  The slot fields stay as they are: the image stream's
// k_pick_next of a frame in flight may read them while this runs.  The matrices come by value (no staging, no host sync).
__global__ void k_reset_seq(DevBuffers d, int seq0, int n, SeqProjection p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    SeqState& s = d.st[seq0 + i];
    s.frame_id = 0; s.n_feat = 0;
    for (int k = 0; k < 9; k++) s.R[k] = (k % 4 == 0);
    for (int k = 0; k < 3; k++) s.t[k] = 0.;
    for (int k = 0; k < 16; k++) s.last_T[k] = (k % 5 == 0);
    if (p.set) {
        for (int k = 0; k < 12; k++) { s.Pl[k] = p.Pl[k]; s.Pr[k] = p.Pr[k]; }
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) s.K[3 * r + c] = p.Pl[4 * r + c];   // K = Pl[:, :3] (vo.cpp:16-25)
    }
}
void launch_reset_seq(const DevBuffers& d, int seq, const SeqProjection& p, hipStream_t st) {
    const int s0 = seq < 0 ? 0 : seq, n = seq < 0 ? d.B : 1;
    hipLaunchKernelGGL(k_reset_seq, dim3((n + 63) / 64), dim3(64), 0, st, d, s0, n, p);
}

// ------------------------------------------------------------------------------------------------
// FAST-9/16 score + strict 3x3 NMS (cv::FAST(img, kps, th, true) at feature_set.cpp:61).
// 64x16 output tile per 256-thread block: 72x24 pixels staged in LDS (3-px circle halo + 1-px NMS
// halo), u8 scores for the 66x18 ring-extended tile in LDS, then NMS.  Survivors either go straight
// into the bucket grid with one 64-bit atomicMax (frame pipeline) or into a dense score map (stage API).
// ------------------------------------------------------------------------------------------------
#define FT_W 64
#define FT_H 16
#define FT_PW (FT_W + 8)
#define FT_PH (FT_H + 8)
#define FT_SW (FT_W + 2)
#define FT_SH (FT_H + 2)

// Bresenham circle r=3 in OpenCV order
#define CIRC_DX {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1}
#define CIRC_DY {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3}

// >= 9 contiguous set bits in a circular 16-bit mask
__device__ __forceinline__ bool run9(unsigned m) {
    unsigned m2 = m | (m << 16);
    unsigned a = m2 & (m2 >> 1);
    unsigned b = a & (a >> 2);
    unsigned c = b & (b >> 4);
    return ((c & (m2 >> 8)) & 0xFFFFu) != 0;
}

// score of the pixel at LDS position (py,px): 0 if not a corner, else max(t, best 9-arc min|diff|) - 1
__device__ __forceinline__ int fast_score(const uint8_t (*pix)[FT_PW + 4], int py, int px, int t) {
    constexpr int cdx[16] = CIRC_DX, cdy[16] = CIRC_DY;
    int v = pix[py][px];
    int dd[16];
    unsigned mb = 0, md = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        int p = pix[py + cdy[k]][px + cdx[k]];
        dd[k] = v - p;
        md |= (unsigned)(p < v - t) << k;       // darker than centre
        mb |= (unsigned)(p > v + t) << k;       // brighter
    }
    if (!run9(mb) && !run9(md)) return 0;
    // sliding 9-window minimum / maximum over the circular sequence
    int best = t, worst = -t;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        int mn = dd[k], mx = dd[k];
#pragma unroll
        for (int j = 1; j < 9; j++) { int e = dd[(k + j) & 15]; mn = e < mn ? e : mn; mx = e > mx ? e : mx; }
        best = mn > best ? mn : best;           // a0 = max(a0, arc-min of (v - p))
        worst = mx < worst ? mx : worst;        // b0 = min(b0, arc-max of (v - p))
    }
    // cornerScore: a0 from the "centre brighter" side, then b0 = min(-a0, arc-max...) ; score = -b0 - 1
    int b0 = -best;
    b0 = worst < b0 ? worst : b0;
    return -b0 - 1;
}

// Bucket::add_feature for capacity 1 as one 64-bit atomicMax; the first candidate of a bucket also counts it into its grid row,
// which lets k_bucket_emit place a row's winners without scanning the rows before it.
__device__ __forceinline__ void bucket_offer(const DevBuffers& d, int seq, int bh, int bw, unsigned long long key) {
    const unsigned long long old = atomicMax(&d.bucket_keys[(size_t)seq * d.NB + bh * d.cfg.buckets_along_width + bw], key);
    if (old == 0ull) atomicAdd(&d.bucket_rowcnt[(size_t)seq * d.cfg.buckets_along_height + bh], 1);
}

// the tracks the feature set already holds, offered to the grid (feature_set.cpp:20-53, 122-124) — the first pass's FAST threads
// share them out before they scan their tiles, the second pass's offer is made by the last block of the first pass's emit
// (mask: the detection mask of the image the tracks lie in, or null — a track it filters out makes no offer, svo.h)
template <bool MASKED = false>
static __device__ __forceinline__ void offer_tracks(const DevBuffers& d, int seq, int fb, int n, int first, int step, const uint8_t* mask = nullptr, int mstride = 0) {
    const BucketGrid g = grid_of(d);
    const float2* xy = d.feat_xy[fb] + (size_t)seq * d.CAP;
    const int* age = d.feat_age[fb] + (size_t)seq * d.CAP;
    const int* str = d.feat_str[fb] + (size_t)seq * d.CAP;
    for (int i = first; i < n; i += step) {
        const float2 p = xy[i];
        const int a = age[i], st = str[i];
        int bh, bw;
        if (!bucket_of(g, p.x, p.y, bh, bw) || a >= g.age_thr) continue;                  // feature_set.cpp:26
        if constexpr (MASKED) if (mask && !mask_keeps(mask, mstride, d.geom.W, d.geom.H, p.x, p.y)) continue;
        bucket_offer(d, seq, bh, bw, make_bucket_key(bucket_score(a, st, g.fast_thr), (unsigned)i, st));
    }
}

// Does detection pass `pass` run for this sequence?  Pass 1 runs where pass 0's emit asked for it.  Pass 0 runs on every frame
// but a sequence's first, which the per-frame reset records in `active` — but the FAST kernels of pass 0 may share a launch with
// the ingest block that performs that reset (k_front_a), so they (before_reset) read frame_id > 0, which the reset computes
// `active` from and does not write; for the same reason they take n_feat, not n_old, as the size of the old set.
static __device__ __forceinline__ bool detect_pass_runs(const SeqState& s, int pass, bool before_reset = false) {
    return pass != 0 ? s.do_second : before_reset ? s.frame_id > 0 : s.active;
}

// ---- where a tile's NMS result goes: sink(gx, gy, score, keep) is called once for every pixel of the tile inside the image ----
// the dense score map (stage API; frame pipeline at features_per_bucket > 1, where the general walk needs the keypoint list)
struct ScoreMapSink {
    uint8_t* score; int W;
    __device__ __forceinline__ void operator()(int gx, int gy, int s, bool keep) const { score[(size_t)gy * W + gx] = keep ? (uint8_t)s : (uint8_t)0; }
};
// straight into the bucket keys (frame pipeline, features_per_bucket == 1): feature_set.cpp:83-87 (age 0, strength = response)
struct BucketSink {
    const DevBuffers& d; int seq, pass;
    __device__ __forceinline__ void operator()(int gx, int gy, int s, bool keep) const {
        const BucketGrid g = grid_of(d);
        int bh, bw;
        if (!keep || !bucket_of(g, (float)gx, (float)gy, bh, bw) || 0 >= g.age_thr) return;
        const unsigned n_old = pass == 0 ? (unsigned)d.st[seq].n_feat : (unsigned)d.st[seq].n_old;   // pass 0: the set is still the old one
        const unsigned order = n_old + (unsigned)(gy * d.geom.W + gx);                               // raster rank keeps cv::FAST's output order
        bucket_offer(d, seq, bh, bw, make_bucket_key(bucket_score(0, s, g.fast_thr), order, s));
    }
};

// the same behind a detection mask: one byte load for a pixel that survived NMS (one in a few hundred), none for the others.
// The survivor keeps its raster rank, so ties break as in the filtered list.  mask == null (a sequence without a mask in a
// launch where others have one): everything is allowed.
struct MaskedBucketSink {
    const DevBuffers& d; int seq, pass; const uint8_t* mask; int mstride;
    __device__ __forceinline__ void operator()(int gx, int gy, int s, bool keep) const {
        if (!keep || (mask && !mask_keeps(mask, mstride, d.geom.W, d.geom.H, (float)gx, (float)gy))) return;
        BucketSink{d, seq, pass}(gx, gy, s, true);
    }
};
// the stage call's score map of the keypoints a mask keeps
struct MaskedScoreMapSink {
    uint8_t* score; int W, H; const uint8_t* mask; int mstride;
    __device__ __forceinline__ void operator()(int gx, int gy, int s, bool keep) const {
        score[(size_t)gy * W + gx] = keep && mask_keeps(mask, mstride, W, H, (float)gx, (float)gy) ? (uint8_t)s : (uint8_t)0;
    }
};

// The tile whose first pixel is (x0, y0) of the W x H image img (rows istride bytes apart): fill, screening, scores, NMS.
template <class Sink>
static __device__ __forceinline__ void fast_tile(const uint8_t* img, int istride, int W, int H, int x0, int y0, int threshold, const Sink& sink) {
    __shared__ __attribute__((aligned(4))) uint8_t pix[FT_PH][FT_PW + 4];
    __shared__ uint8_t sc[FT_SH][FT_SW + 2];
    __shared__ unsigned short cand[FT_SH * FT_SW];               // screened pixels of the tile (order is irrelevant)
    __shared__ int ncand;
    if (threshold < 0) threshold = 0;
    if (threshold > 255) threshold = 255;
    if (x0 >= 4 && y0 >= 4 && x0 - 4 + FT_PW <= W && y0 - 4 + FT_PH <= H) {
        // interior tile: 18 unaligned dword loads per row instead of 72 guarded byte loads
        static_assert(FT_PW % 4 == 0, "tile rows are whole dwords");
        constexpr int DPR = FT_PW / 4;
        for (int i = threadIdx.x; i < DPR * FT_PH; i += 256) {
            int py = i / DPR, c = i - py * DPR;
            const unsigned v = reinterpret_cast<const UD*>(img + (size_t)(y0 - 4 + py) * istride + (x0 - 4) + 4 * c)->v;
            *reinterpret_cast<unsigned*>(&pix[py][4 * c]) = v;
        }
    } else {
        for (int i = threadIdx.x; i < FT_PH * FT_PW; i += 256) {
            int py = i / FT_PW, px = i - py * FT_PW;
            int gx = x0 - 4 + px, gy = y0 - 4 + py;
            pix[py][px] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? img[(size_t)gy * istride + gx] : (uint8_t)0;
        }
    }
    if (threadIdx.x == 0) ncand = 0;
    __syncthreads();
    // Screening: a 9-arc of the 16-pixel circle contains at least one pixel of every antipodal pair, so a corner needs a
    // darker (or a brighter) member in each of the pairs (0,8) and (4,12).  Typically ~7 % of the pixels pass (th = 20);
    // only those are queued for the full 16-pixel test, which then runs on densely packed waves.
    for (int i = threadIdx.x; i < FT_SH * FT_SW; i += 256) {
        int sy = i / FT_SW, sx = i - sy * FT_SW;
        int gx = x0 - 1 + sx, gy = y0 - 1 + sy;
        sc[sy][sx] = 0;
        if (gx >= 3 && gx < W - 3 && gy >= 3 && gy < H - 3) {
            const int py = sy + 3, px = sx + 3;
            const int v = pix[py][px], lo = v - threshold, hi = v + threshold;
            const int a = pix[py + 3][px], b = pix[py - 3][px], c = pix[py][px + 3], e = pix[py][px - 3];   // circle 0, 8, 4, 12
            const bool dark = (a < lo || b < lo) && (c < lo || e < lo);
            const bool bright = (a > hi || b > hi) && (c > hi || e > hi);
            if (dark || bright) cand[atomicAdd(&ncand, 1)] = (unsigned short)i;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < ncand; k += 256) {
        const int i = cand[k];
        int sy = i / FT_SW, sx = i - sy * FT_SW;
        sc[sy][sx] = (uint8_t)fast_score(pix, sy + 3, sx + 3, threshold);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < FT_W * FT_H; i += 256) {
        int oy = i / FT_W, ox = i - oy * FT_W;
        int gx = x0 + ox, gy = y0 + oy;
        if (gx >= W || gy >= H) continue;
        int s = sc[oy + 1][ox + 1];
        bool keep = s != 0 &&
                    s > sc[oy + 1][ox] && s > sc[oy + 1][ox + 2] &&
                    s > sc[oy][ox] && s > sc[oy][ox + 1] && s > sc[oy][ox + 2] &&
                    s > sc[oy + 2][ox] && s > sc[oy + 2][ox + 1] && s > sc[oy + 2][ox + 2];
        sink(gx, gy, s, keep);
    }
}

// The frame side of a FAST block: what it scans for sequence slot bz — FAST runs on the PREVIOUS left image (vo.cpp:325), for a
// BGR context on the byte image cv::FAST really scans, else on level 0 of the pyramid, which carries its border (istride) —
// or false if the pass does not run for the sequence.  Pass 0 of a capacity-1 context (`offer`): the existing tracks enter the
// grid here (no launch of their own), this thread's share being first, first + step, ...
struct FastFrame { int seq; const uint8_t* img; int istride; };
template <bool MASKED = false>
static __device__ __forceinline__ bool fast_frame_begin(const DevBuffers& d, int pass, int bz, bool offer, int first, int step, FastFrame& f,
                                                        const MaskArgs* m = nullptr) {
    f.seq = seq_of(d, bz);
    const SeqState& s = d.st[f.seq];
    if (!detect_pass_runs(s, pass, true)) return false;
    f.img = d.CN == 3 ? d.fastimg + fastimg_index(d, f.seq, s.slot_img_t0) : d.pyr + pyr_index(d, f.seq, s.slot_img_t0, 0) + d.geom.lv[0].off;
    f.istride = d.CN == 3 ? d.geom.W : d.geom.lv[0].stride;
    if constexpr (MASKED) { if (offer && pass == 0) offer_tracks<true>(d, f.seq, s.feat_buf, s.n_feat, first, step, m->rows[f.seq], m->stride); }
    else if (offer && pass == 0) offer_tracks(d, f.seq, s.feat_buf, s.n_feat, first, step);
    return true;
}
// tile (bx, by) of the fx x fy tiles of sequence slot bz, survivors to the bucket keys: a block of k_fast<0> or of k_front_a
static __device__ __forceinline__ void fast_frame_block(const DevBuffers& d, int pass, int threshold, int bx, int by, int bz, int fx, int fy) {
    FastFrame f;
    if (!fast_frame_begin(d, pass, bz, true, (by * fx + bx) * 256 + threadIdx.x, fx * fy * 256, f)) return;
    fast_tile(f.img, f.istride, d.geom.W, d.geom.H, bx * FT_W, by * FT_H, threshold, BucketSink{d, f.seq, pass});
}
// MODE 0: survivors go straight to the bucket keys (features_per_bucket == 1).  MODE 2: to the sequence's score map
// (features_per_bucket > 1).  One block per tile and sequence slot.
template <int MODE>
__global__ __launch_bounds__(256) void k_fast(DevBuffers d, int pass, int threshold) {
    static_assert(MODE == 0 || MODE == 2, "the stage call's score map is k_fast_score_map");
    if (MODE == 0) { fast_frame_block(d, pass, threshold, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, gridDim.y); return; }
    FastFrame f;
    if (!fast_frame_begin(d, pass, blockIdx.z, false, 0, 0, f)) return;
    const int W = d.geom.W, H = d.geom.H;
    fast_tile(f.img, f.istride, W, H, blockIdx.x * FT_W, blockIdx.y * FT_H, threshold, ScoreMapSink{d.score + (size_t)f.seq * W * H, W});
}
// one packed image -> score map (stage API)
__global__ __launch_bounds__(256) void k_fast_score_map(const uint8_t* img, int w, int h, int threshold, uint8_t* score) {
    fast_tile(img, w, w, h, blockIdx.x * FT_W, blockIdx.y * FT_H, threshold, ScoreMapSink{score, w});
}

// ---- FAST pass 0 of a plain many-sequence context (no masks, no ids, one feature per bucket): k_fast_batch.  The same tile steps
// as fast_tile with the same pixel rules — same candidates, same scores, same survivors, same keys — re-shaped for a thousand
// images per launch, where the tiles' turnover is the cost:
//  - a 64 x 32 tile: the 4-pixel halo is 41 % on top of the tile instead of 69 %, and a tile queues ~160 candidates, so the
//    scoring rounds run on two or three full waves instead of one wave and a quarter;
//  - screening takes FOUR pixels per lane from five LDS dwords (the dword of the pixels, its two neighbours, the rows 3 above and
//    below) instead of five byte reads per pixel, and a wave queues its candidates with a ballot and ONE LDS add;
//  - NMS visits the queued candidates only: no other pixel can have a score, and the bucket sink ignores a pixel that is not kept;
//  - the score runs on 16-bit pairs (fast_score_pk): the same integers from a sixth of the instructions.
// fast_score on packed pairs.  With d[k] = v - circle[k], a pixel is a corner iff some 9-arc has all d > t (run9 of the "darker" mask)
// or all d < -t (the "brighter" mask), i.e. iff  A = max_k min_{j<9} d[k+j] > t  or  B = min_k max_{j<9} d[k+j] < -t,  and
// fast_score's result is max(max(t, A), -min(-t, B)) - 1: the masks and the score are one computation.  Register k holds the pair
// (d[k], d[k+8]), so the pair of index k + 8 is register k with its halves swapped and the windows starting at k and at k + 8
// slide together: windows of 2, 4, 8 by doubling, the ninth element last — 32 v_pk_min and 32 v_pk_max for all sixteen arcs
// (fast_score: 16 x 8 of each, after 64 instructions of mask building).  |d| <= 255: exact in 16 bits.
typedef short fs_s2 __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ fs_s2 fs_swap(fs_s2 a) { return __builtin_shufflevector(a, a, 1, 0); }
template <bool MAX> static __device__ __forceinline__ fs_s2 fs_pick(fs_s2 a, fs_s2 b) { return MAX ? __builtin_elementwise_max(a, b) : __builtin_elementwise_min(a, b); }
// windows of 2 S from windows of S: out[k] = pick(in[k], in[k + S]), indices 8 .. 15 being the swapped registers 0 .. 7
template <bool MAX, int S>
static __device__ __forceinline__ void fs_double(const fs_s2 (&in)[8], fs_s2 (&out)[8]) {
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = fs_pick<MAX>(in[k], k + S < 8 ? in[k + S] : fs_swap(in[k + S - 8]));
}
template <bool MAX>
static __device__ __forceinline__ int fs_arcs(const fs_s2 (&d)[8]) {   // MAX = false: A above; true: B
    fs_s2 a[8], b[8];
    fs_double<MAX, 1>(d, a); fs_double<MAX, 2>(a, b); fs_double<MAX, 4>(b, a);
#pragma unroll
    for (int k = 0; k < 8; k++) a[k] = fs_pick<MAX>(a[k], fs_swap(d[k]));          // the ninth element: d[k + 8]
    fs_s2 r = a[0];
#pragma unroll
    for (int k = 1; k < 8; k++) r = fs_pick<!MAX>(r, a[k]);
    return MAX ? (r.x < r.y ? r.x : r.y) : (r.x > r.y ? r.x : r.y);
}
static __device__ __forceinline__ int fast_score_pk(const uint8_t (*pix)[FT_PW + 4], int py, int px, int t) {
    constexpr int cdx[16] = CIRC_DX, cdy[16] = CIRC_DY;
    const short v = pix[py][px];
    fs_s2 d[8];
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = fs_s2{v, v} - fs_s2{(short)pix[py + cdy[k]][px + cdx[k]], (short)pix[py + cdy[k + 8]][px + cdx[k + 8]]};
    const int A = fs_arcs<false>(d), B = fs_arcs<true>(d);
    if (A <= t && B >= -t) return 0;
    const int best = A > t ? A : t, worst = B < -t ? B : -t;
    return (best > -worst ? best : -worst) - 1;
}
#define FB_W 64
#define FB_H 32
#define FB_PH (FB_H + 8)
#define FB_SH (FB_H + 2)
static_assert(FB_W == FT_W, "fast_score reads rows of FT_PW + 4 bytes");
static __device__ __forceinline__ void fast_tile_batch(const uint8_t* img, int istride, int W, int H, int x0, int y0, int threshold, const BucketSink& sink) {
    __shared__ __attribute__((aligned(4))) uint8_t pix[FB_PH][FT_PW + 4];
    __shared__ __attribute__((aligned(4))) uint8_t sc[FB_SH][FT_SW + 2];
    __shared__ unsigned short cand[FB_SH * FT_SW];
    __shared__ int ncand;
    constexpr int DPR = FT_PW / 4;                                    // dwords of a pixel row
    if (threshold < 0) threshold = 0;
    if (threshold > 255) threshold = 255;
    if (x0 >= 4 && y0 >= 4 && x0 - 4 + FT_PW <= W && y0 - 4 + FB_PH <= H) {
        for (int i = threadIdx.x; i < DPR * FB_PH; i += 256) {
            const int py = i / DPR, c = i - py * DPR;
            *reinterpret_cast<unsigned*>(&pix[py][4 * c]) = reinterpret_cast<const UD*>(img + (size_t)(y0 - 4 + py) * istride + (x0 - 4) + 4 * c)->v;
        }
    } else {
        for (int i = threadIdx.x; i < FB_PH * FT_PW; i += 256) {
            const int py = i / FT_PW, px = i - py * FT_PW;
            const int gx = x0 - 4 + px, gy = y0 - 4 + py;
            pix[py][px] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? img[(size_t)gy * istride + gx] : (uint8_t)0;
        }
    }
    static_assert(sizeof(sc) % 4 == 0, "the score tile is cleared a dword at a time");
    for (int i = threadIdx.x; i < (int)sizeof(sc) / 4; i += 256) reinterpret_cast<unsigned*>(&sc[0][0])[i] = 0u;
    if (threadIdx.x == 0) ncand = 0;
    __syncthreads();
    // Screening (fast_tile's rule).  Lane item (sy, c): the four pixels of dword c of pixel row sy + 3, i.e. score-tile columns
    // sx = 4 c - 3 .. 4 c; every lane of a wave takes part in the ballots, also where its item or its pixels lie outside.
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < FB_SH * DPR; base += 256) {
        const int i = base + threadIdx.x, sy = i / DPR, c = i - sy * DPR;
        bool pass[4] = {false, false, false, false};
        if (i < FB_SH * DPR) {
            const int gy = y0 - 1 + sy;
            const unsigned* row = reinterpret_cast<const unsigned*>(&pix[sy + 3][0]);
            const unsigned ctr = row[c], prv = c > 0 ? row[c - 1] : 0u, nxt = row[c + 1];                    // (row[DPR] is the row's padding: read, never used)
            const unsigned lft = __builtin_amdgcn_alignbyte(ctr, prv, 1), rgt = __builtin_amdgcn_alignbyte(nxt, ctr, 3);   // the pixels 3 to the left / right of the four
            const unsigned dn = reinterpret_cast<const unsigned*>(&pix[sy + 6][0])[c], up = reinterpret_cast<const unsigned*>(&pix[sy][0])[c];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int sx = 4 * c - 3 + j, gx = x0 - 1 + sx;
                if (sx >= 0 && sx < FT_SW && gx >= 3 && gx < W - 3 && gy >= 3 && gy < H - 3) {
                    const int v = (ctr >> (8 * j)) & 255, lo = v - threshold, hi = v + threshold;
                    const int a = (dn >> (8 * j)) & 255, b = (up >> (8 * j)) & 255, cc = (rgt >> (8 * j)) & 255, e = (lft >> (8 * j)) & 255;   // circle 0, 8, 4, 12
                    const bool dark = (a < lo || b < lo) && (cc < lo || e < lo);
                    const bool bright = (a > hi || b > hi) && (cc > hi || e > hi);
                    pass[j] = dark || bright;
                }
            }
        }
        unsigned long long m[4];
        int n = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) { m[j] = __ballot(pass[j]); n += __popcll(m[j]); }
        if (n == 0) continue;                                         // wave-uniform
        int at = 0;
        if (lane == 0) at = atomicAdd(&ncand, n);
        at = __shfl(at, 0);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (pass[j]) cand[at + __popcll(m[j] & ((1ull << lane) - 1ull))] = (unsigned short)(sy * FT_SW + 4 * c - 3 + j);
            at += __popcll(m[j]);
        }
    }
    __syncthreads();
    const int nc = __builtin_amdgcn_readfirstlane(ncand);           // block-uniform: a scalar register
    for (int k = threadIdx.x; k < nc; k += 256) {
        const int i = cand[k], sy = i / FT_SW, sx = i - sy * FT_SW;
        sc[sy][sx] = (uint8_t)fast_score_pk(pix, sy + 3, sx + 3, threshold);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nc; k += 256) {
        const int i = cand[k], sy = i / FT_SW, sx = i - sy * FT_SW;
        const int gx = x0 + sx - 1, gy = y0 + sy - 1;
        if (sx < 1 || sx > FB_W || sy < 1 || sy > FB_H || gx >= W || gy >= H) continue;   // the ring around the tile: a neighbour's pixel
        const int s = sc[sy][sx];
        const bool keep = s != 0 &&
                          s > sc[sy][sx - 1] && s > sc[sy][sx + 1] &&
                          s > sc[sy - 1][sx - 1] && s > sc[sy - 1][sx] && s > sc[sy - 1][sx + 1] &&
                          s > sc[sy + 1][sx - 1] && s > sc[sy + 1][sx] && s > sc[sy + 1][sx + 1];
        sink(gx, gy, s, keep);
    }
}
__global__ __launch_bounds__(256) void k_fast_batch(DevBuffers d, int pass, int threshold) {
    FastFrame f;
    if (!fast_frame_begin(d, pass, blockIdx.z, true, (blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x, gridDim.x * gridDim.y * 256, f)) return;
    fast_tile_batch(f.img, f.istride, d.geom.W, d.geom.H, blockIdx.x * FB_W, blockIdx.y * FB_H, threshold, BucketSink{d, f.seq, pass});
}

// The SECOND detection pass of a many-sequence context: launched every frame, needed by a sequence that kept < 100 features (vo.cpp:327)
// — on a healthy scene by none.  One block per tile and sequence (123 000 blocks at 256 sequences) costs 0.15-0.25 ms on the frame's
// critical chain just to look at do_second and leave; here a sequence gets FAST_STRIDED_BLOCKS blocks that walk its tiles.
#define FAST_STRIDED_BLOCKS 32
__global__ __launch_bounds__(256) void k_fast_strided(DevBuffers d, int pass, int threshold, int fx, int fy) {
    FastFrame f;
    if (!fast_frame_begin(d, pass, blockIdx.z, true, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256, f)) return;
    for (int t = blockIdx.x; t < fx * fy; t += gridDim.x) {
        fast_tile(f.img, f.istride, d.geom.W, d.geom.H, (t % fx) * FT_W, (t / fx) * FT_H, threshold, BucketSink{d, f.seq, pass});
        __syncthreads();                                              // the tile arrays in LDS are reused by the next tile
    }
}

// ---- detection masks (svo.h, svo_set_detection_mask): the two FAST kernels of the capacity-1 pipeline with MaskArgs.  A sequence
// whose row is null is offered and scanned unfiltered in the same launch.  The emit kernels are the plain ones: a filtered
// entry made no offer, and pass 1's re-offer of the new set (bucket_emit_body) offers a set the mask has already been applied to.
static __device__ __forceinline__ void fast_tile_masked(const DevBuffers& d, const FastFrame& f, int pass, int threshold, int x0, int y0, const uint8_t* mask, int mstride) {
    fast_tile(f.img, f.istride, d.geom.W, d.geom.H, x0, y0, threshold, MaskedBucketSink{d, f.seq, pass, mask, mstride});
}
__global__ __launch_bounds__(256) void k_fast_masked(DevBuffers d, MaskArgs m, int pass, int threshold) {
    FastFrame f;
    if (!fast_frame_begin<true>(d, pass, blockIdx.z, true, (blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x, gridDim.x * gridDim.y * 256, f, &m)) return;
    fast_tile_masked(d, f, pass, threshold, blockIdx.x * FT_W, blockIdx.y * FT_H, m.rows[f.seq], m.stride);
}
__global__ __launch_bounds__(256) void k_fast_strided_masked(DevBuffers d, MaskArgs m, int pass, int threshold, int fx, int fy) {
    FastFrame f;
    if (!fast_frame_begin<true>(d, pass, blockIdx.z, true, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256, f, &m)) return;
    const uint8_t* mask = m.rows[f.seq];
    for (int t = blockIdx.x; t < fx * fy; t += gridDim.x) {
        fast_tile_masked(d, f, pass, threshold, (t % fx) * FT_W, (t / fx) * FT_H, mask, m.stride);
        __syncthreads();                                              // the tile arrays in LDS are reused by the next tile
    }
}
__global__ __launch_bounds__(256) void k_fast_score_map_masked(const uint8_t* img, int w, int h, int threshold, const uint8_t* mask, int mstride, uint8_t* score) {
    fast_tile(img, w, w, h, blockIdx.x * FT_W, blockIdx.y * FT_H, threshold, MaskedScoreMapSink{score, w, h, mask, mstride});
}

static dim3 fast_grid(int w, int h, int n_seq) { return dim3((w + FT_W - 1) / FT_W, (h + FT_H - 1) / FT_H, n_seq); }
static dim3 fast_grid(const DevBuffers& d) { return fast_grid(d.geom.W, d.geom.H, launch_seqs(d)); }

void launch_fast_score_map(const uint8_t* img_dev, int w, int h, int threshold, uint8_t* score_dev, hipStream_t st) {
    hipLaunchKernelGGL(k_fast_score_map, fast_grid(w, h, 1), dim3(256), 0, st, img_dev, w, h, threshold, score_dev);
}

// ---- a score map as the raster-ordered keypoint list (cv::FAST's output order + KeyPoint::convert, feature_set.cpp:62-66):
// one 64-lane block per image row counts its keypoints, one thread turns the counts into offsets, one block per row emits ----
static __device__ __forceinline__ int score_row_count(const uint8_t* row, int w) {
    int cnt = 0;
    for (int x = threadIdx.x; x < w; x += 64) cnt += row[x] != 0;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    return cnt;
}
static __device__ __forceinline__ int scan_rows(int* rows, int h, int acc) {       // serial; h is a few hundred
    for (int y = 0; y < h; y++) { const int c = rows[y]; rows[y] = acc; acc += c; }
    return acc;
}
// store(idx, x, score) for every keypoint of the row whose list position idx (base + its rank in the row) is below cap
template <class Store>
static __device__ __forceinline__ void score_row_emit(const uint8_t* row, int w, int base, int cap, const Store& store) {
    for (int x0 = 0; x0 < w; x0 += 64) {
        const int x = x0 + threadIdx.x;
        const int s = x < w ? row[x] : 0;
        const unsigned long long m = __ballot(s != 0);
        if (s) {
            const int idx = base + __popcll(m & ((1ull << threadIdx.x) - 1ull));
            if (idx < cap) store(idx, x, s);
        }
        base += __popcll(m);
    }
}

// svo_fast_detect: (xy, response) per keypoint
__global__ void k_score_row_count(const uint8_t* score, int w, int* row_counts) {
    const int cnt = score_row_count(score + (size_t)blockIdx.x * w, w);
    if (threadIdx.x == 0) row_counts[blockIdx.x] = cnt;
}
__global__ void k_scan_rows(int* row_counts, int h, int* n_out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *n_out = scan_rows(row_counts, h, 0);
}
__global__ void k_score_row_emit(const uint8_t* score, int w, const int* row_off, int cap, float2* xy, float* resp) {
    const int y = blockIdx.x;
    score_row_emit(score + (size_t)y * w, w, row_off[y], cap, [=](int idx, int x, int s) { xy[idx] = make_float2((float)x, (float)y); resp[idx] = (float)s; });
}
void launch_fast_score_map_masked(const uint8_t* img_dev, int w, int h, int threshold, const uint8_t* mask_dev, int mask_stride, uint8_t* score_dev, hipStream_t st) {
    hipLaunchKernelGGL(k_fast_score_map_masked, fast_grid(w, h, 1), dim3(256), 0, st, img_dev, w, h, threshold, mask_dev, mask_stride, score_dev);
}
void launch_score_compact(const uint8_t* score_dev, int w, int h, int cap, int* row_counts_dev, float2* xy_dev, float* resp_dev, int* n_dev, hipStream_t st) {
    hipLaunchKernelGGL(k_score_row_count, dim3(h), dim3(64), 0, st, score_dev, w, row_counts_dev);
    hipLaunchKernelGGL(k_scan_rows, dim3(1), dim3(64), 0, st, row_counts_dev, h, n_dev);
    hipLaunchKernelGGL(k_score_row_emit, dim3(h), dim3(64), 0, st, score_dev, w, row_counts_dev, cap, xy_dev, resp_dev);
}

// ------------------------------------------------------------------------------------------------
// Bucketing for features_per_bucket == 1 (the reference default, vo.h:65).
// Bucket::add_feature's "first in, replace the minimum iff strictly better" with one slot is
// argmax(score) with ties -> lowest input index, i.e. one 64-bit atomicMax per candidate with
// key = (score, ~input_index, strength).  Input order = existing tracks first, then the new FAST
// hits in raster order (feature_set.cpp:83-87).  Emission is bucket-raster order (:132-146).
// ------------------------------------------------------------------------------------------------
// Emit the winners in bucket-raster order (feature_set.cpp:132-146): one block per (grid row, sequence).  The rows' occupancy
// counts (bucket_offer) give a block its first output position; inside the row a ballot scan orders the winners.  Each block
// zeroes the keys it has read and the LAST block of a sequence (ticket) zeroes the row counts and publishes the new feature set,
// so keys, counts and tickets are all zero again when the next pass or frame starts — no clearing launch anywhere.  If the first
// pass kept too few features (vo.cpp:327) that last block also offers the new set to the grid for the second pass.
#define EMIT_THREADS 256
#define EMIT_WAVES (EMIT_THREADS / 64)
// IDS (svo.h, the identity rule, step 1): the winner's `order` is the only place its source rank exists — an entry of the old list
// keeps its id, a fresh FAST hit at output position pos gets next_id + pos — and the publishing block advances next_id by the
// count.  Every block reads next_id before it takes its ticket, the publisher writes it after the last ticket.
template <bool IDS = false>
static __device__ __forceinline__ void bucket_emit_body(const DevBuffers& d, int pass, int row, int b, int n_rows, const IdArgs* ia = nullptr) {
    const int seq = seq_of(d, b);
    SeqState& s = d.st[seq];
    if (!detect_pass_runs(s, pass)) return;
    __shared__ int sh_before[EMIT_WAVES], sh_all[EMIT_WAVES], sh_cnt[EMIT_WAVES], sh_last;
    const int fb = s.feat_buf, n_old = s.n_old, W = d.geom.W;
    const int baw = d.cfg.buckets_along_width, bah = d.cfg.buckets_along_height;
    unsigned long long* keys = d.bucket_keys + (size_t)seq * d.NB + (size_t)row * baw;
    int* rowcnt = d.bucket_rowcnt + (size_t)seq * bah;
    const float2* oxy = d.feat_xy[fb] + (size_t)seq * d.CAP;
    const int* oage = d.feat_age[fb] + (size_t)seq * d.CAP;
    const int* ostr = d.feat_str[fb] + (size_t)seq * d.CAP;
    float2* nxy = d.feat_xy[fb ^ 1] + (size_t)seq * d.CAP;
    int* nage = d.feat_age[fb ^ 1] + (size_t)seq * d.CAP;
    int* nstr = d.feat_str[fb ^ 1] + (size_t)seq * d.CAP;
    long long id_base = 0; const long long* oid = nullptr; long long* nid = nullptr;
    if constexpr (IDS) { id_base = ia->next_id[seq]; oid = ia->feat_id[fb] + (size_t)seq * d.CAP; nid = ia->feat_id[fb ^ 1] + (size_t)seq * d.CAP; }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // winners in the rows before this one, and in all rows
    int before = 0, all = 0;
    for (int r = threadIdx.x; r < bah; r += EMIT_THREADS) { const int c = rowcnt[r]; all += c; if (r < row) before += c; }
    for (int o = 32; o > 0; o >>= 1) { before += __shfl_xor(before, o); all += __shfl_xor(all, o); }
    if (lane == 0) { sh_before[wv] = before; sh_all[wv] = all; }
    __syncthreads();
    before = 0; all = 0;
    for (int w = 0; w < EMIT_WAVES; w++) { before += sh_before[w]; all += sh_all[w]; }
    int run = before;
    for (int b0 = 0; b0 < baw; b0 += EMIT_THREADS) {
        const int bw = b0 + threadIdx.x;
        unsigned long long k = 0ull;
        if (bw < baw) { k = keys[bw]; if (k != 0ull) keys[bw] = 0ull; }
        const unsigned long long m = __ballot(k != 0ull);
        __syncthreads();                                              // sh_cnt of the previous chunk has been read
        if (lane == 0) sh_cnt[wv] = __popcll(m);
        __syncthreads();
        int pos = run + __popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wv; w++) pos += sh_cnt[w];
        for (int w = 0; w < EMIT_WAVES; w++) run += sh_cnt[w];
        if (k != 0ull && pos < d.CAP) {
            const unsigned order = 0xFFFFFFFFu - (unsigned)((k >> 16) & 0xFFFFFFFFull);
            if constexpr (IDS) nid[pos] = order < (unsigned)n_old ? oid[order] : id_base + pos;
            if (order < (unsigned)n_old) { nxy[pos] = oxy[order]; nage[pos] = oage[order]; nstr[pos] = ostr[order]; }
            else {
                const unsigned pixi = order - (unsigned)n_old;
                const int y = (int)(pixi / (unsigned)W), x = (int)(pixi - (unsigned)y * (unsigned)W);
                nxy[pos] = make_float2((float)x, (float)y); nage[pos] = 0; nstr[pos] = (int)(k & 0xFFFFull);
            }
        }
    }
    // ---- the last block of the sequence to get here publishes the result.  Every block has read the state it needs by now, so
    // the ticket needs no fence — except when a second pass follows (every block can tell: it knows the total), where the last
    // block reads the features the others wrote.  (An agent-scope fence writes back and invalidates the XCD's L2: thousands of
    // them per frame cost the LK kernel of the other context a third of its speed.)
    const int total = all < d.CAP ? all : d.CAP;
    const bool second = pass == 0 && total < d.cfg.pre_matching_feature_threshold;               // vo.cpp:327
    if (second) __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) sh_last = atomicAdd(&d.emit_ticket[seq], 1) == n_rows - 1;
    __syncthreads();
    if (!sh_last) return;
    if (second) __threadfence();
    for (int r = threadIdx.x; r < bah; r += EMIT_THREADS) rowcnt[r] = 0;
    if (threadIdx.x == 0) {
        d.emit_ticket[seq] = 0;
        s.n_feat = total; s.feat_buf = fb ^ 1;
        s.stats.n_after_detect = total;
        if (pass == 0) { s.do_second = second; if (second) s.n_old = total; }
        else s.stats.second_pass = 1;
        if constexpr (IDS) ia->next_id[seq] = id_base + total;
    }
    if (second) {                                                     // block-uniform
        __threadfence();
        __syncthreads();
        offer_tracks(d, seq, fb ^ 1, total, threadIdx.x, EMIT_THREADS);
    }
}
__global__ __launch_bounds__(EMIT_THREADS) void k_bucket_emit(DevBuffers d, int pass) { bucket_emit_body(d, pass, blockIdx.x, blockIdx.y, gridDim.x); }
// the same with EMIT_STRIDED_BLOCKS blocks per sequence walking the grid rows (the second pass of many-sequence contexts, see
// k_fast_strided): the ticket still counts ROWS, so the block that finishes the last row publishes
#define EMIT_STRIDED_BLOCKS 8
__global__ __launch_bounds__(EMIT_THREADS) void k_bucket_emit_strided(DevBuffers d, int pass, int n_rows) {
    if (!detect_pass_runs(d.st[seq_of(d, blockIdx.y)], pass)) return;
    for (int row = blockIdx.x; row < n_rows; row += gridDim.x) {
        bucket_emit_body(d, pass, row, blockIdx.y, n_rows);
        __syncthreads();
    }
}

// the ids builds of the two emit kernels (svo_set_track_output); masked and plain detection share them, as they share the emit
__global__ __launch_bounds__(EMIT_THREADS) void k_bucket_emit_ids(DevBuffers d, IdArgs ia, int pass) {
    bucket_emit_body<true>(d, pass, blockIdx.x, blockIdx.y, gridDim.x, &ia);
}
__global__ __launch_bounds__(EMIT_THREADS) void k_bucket_emit_strided_ids(DevBuffers d, IdArgs ia, int pass, int n_rows) {
    if (!detect_pass_runs(d.st[seq_of(d, blockIdx.y)], pass)) return;
    for (int row = blockIdx.x; row < n_rows; row += gridDim.x) {
        bucket_emit_body<true>(d, pass, row, blockIdx.y, n_rows, &ia);
        __syncthreads();
    }
}

// ---- the front of a lone stream's frame in two launches instead of four.  Ingest + pyramid and detection are independent
// chains (FAST runs on the PREVIOUS left image, vo.cpp:325): on a nearly empty GPU their kernels ran one after the other, each
// a few microseconds of work behind a launch.  k_front_a = {ingest + level 1 (with the per-frame reset)  ||  FAST pass 0},
// k_front_b = {levels 2 and 3  ||  emit of pass 0}: blocks of both kinds in one grid, told apart by their linear index; the
// two halves of a launch touch disjoint data (detect_pass_runs).  Lone-stream contexts only (SVO_LONE_MAX_SEQ): with many
// sequences every kernel fills the GPU by itself and the separate launches stay.  k_front_a_grey: converting contexts (BPP > 1).
static_assert(EMIT_THREADS == 256, "k_front_b runs emit blocks beside 256-thread pyramid blocks");
template <int BPP, bool RECT>
static __device__ __forceinline__ void front_a_body(const DevBuffers& d, const uint8_t* const* srcs, int stride, int ax, int ay, int n_a, int fx, int fy, int threshold) {
    const int i = blockIdx.x;
    if (i < n_a) { ingest_pyr1_body<PD_TW, PD_TH, RECT, BPP>(d, srcs, stride, PYR_BEGIN, i % ax, (i / ax) % ay, i / (ax * ay)); return; }
    const int j = i - n_a;
    fast_frame_block(d, 0, threshold, j % fx, (j / fx) % fy, j / (fx * fy), fx, fy);
}
template <bool RECT>
__global__ __launch_bounds__(256) void k_front_a(DevBuffers d, const uint8_t* const* srcs, int stride, int ax, int ay, int n_a, int fx, int fy, int threshold) {
    front_a_body<1, RECT>(d, srcs, stride, ax, ay, n_a, fx, fy, threshold);
}
template <int BPP, bool RECT>
__global__ __launch_bounds__(256) void k_front_a_grey(DevBuffers d, const uint8_t* const* srcs, int stride, int ax, int ay, int n_a, int fx, int fy, int threshold) {
    front_a_body<BPP, RECT>(d, srcs, stride, ax, ay, n_a, fx, fy, threshold);
}
__global__ __launch_bounds__(256) void k_front_b(DevBuffers d, int px, int py, int n_p, int n_rows) {
    const int i = blockIdx.x;
    if (i < n_p) { pyrdown2_body(d, 1, PYR_T1, i % px, (i / px) % py, i / (px * py)); return; }
    const int j = i - n_p;
    bucket_emit_body(d, 0, j % n_rows, j / n_rows, n_rows);
}
// true if the fused front applies to this context (then it has been launched): single-channel, four pyramid levels or more,
// one feature per bucket, a lone stream
bool launch_front_fused(const DevBuffers& d, const uint8_t* const* left_right_dev_ptrs, int stride, hipStream_t st) {
    static const bool off = getenv("SVO_FRONT_FUSED") && atoi(getenv("SVO_FRONT_FUSED")) == 0;
    if (off || d.B > SVO_LONE_MAX_SEQ || d.CN != 1 || d.geom.nlevels < 4 || d.cfg.features_per_bucket != 1) return false;
    const int ns = launch_seqs(d);
    const int ax = (d.geom.lv[1].w + PD_TW - 1) / PD_TW, ay = (d.geom.lv[1].h + PD_TH - 1) / PD_TH, n_a = ax * ay * ns * 2;
    const dim3 f = fast_grid(d);
    const int fx = f.x, fy = f.y, n_f = fx * fy * ns;
    if (d.in.bpp > 1) {
        with_bpp(d.in.bpp, [&](auto b) {
            constexpr int BPP = decltype(b)::value;
            const auto front_a = d.rmap ? k_front_a_grey<BPP, true> : k_front_a_grey<BPP, false>;
            hipLaunchKernelGGL(front_a, dim3(n_a + n_f), dim3(256), 0, st, d, left_right_dev_ptrs, stride, ax, ay, n_a, fx, fy, d.cfg.fast_threshold);
        });
    } else {
        const auto front_a = d.rmap ? k_front_a<true> : k_front_a<false>;
        hipLaunchKernelGGL(front_a, dim3(n_a + n_f), dim3(256), 0, st, d, left_right_dev_ptrs, stride, ax, ay, n_a, fx, fy, d.cfg.fast_threshold);
    }
    const int px = (d.geom.lv[3].w + P2_TW - 1) / P2_TW, py = (d.geom.lv[3].h + P2_TH - 1) / P2_TH, n_p = px * py * ns * 2;
    const int n_rows = d.cfg.buckets_along_height;
    hipLaunchKernelGGL(k_front_b, dim3(n_p + n_rows * ns), dim3(256), 0, st, d, px, py, n_p, n_rows);
    launch_pyramid_from(d, 4, st, PYR_T1);                                    // a fifth level and beyond (cfg3)
    launch_pad_pyramid(d, st, PYR_T1);
    launch_detect(d, 1, -1, st);                                      // the second pass exits at once unless needed (vo.cpp:327-332)
    return true;
}

// ------------------------------------------------------------------------------------------------
// General bucketing (any features_per_bucket): FeatureSet::appendFeaturesFromImage as written (feature_set.cpp:75-89).  A pass's
// input list = existing tracks, then cv::FAST's keypoints in raster order (age 0, strength = response), walked in that order
// through Bucket::add_feature (fill, then replace the first minimum iff strictly better, :20-53), emitted in bucket-raster
// order (:132-146).  One thread per bucket walks the whole list: O(N x buckets), the price of a capacity the reference itself
// only uses in its unit tests (main.cpp:125, 152-157); the default capacity 1 never comes here.  The walk and the emit are
// written once, for one grid and one list; the frame pipeline (k_gen_*: per sequence, from DevBuffers) and the stage call
// svo_bucket_filter (k_bucket_walk / k_bucket_order_emit: the caller's list) wrap them.
// ------------------------------------------------------------------------------------------------
// bucket b of the grid: its slots (slot_* + b * per) and their number slot_n[b] from the n candidates
static __device__ __forceinline__ void bucket_walk(const BucketGrid& g, int per, int n, const float2* xy, const int* age, const int* str,
                                                   float2* slot_xy, int* slot_age, int* slot_str, int* slot_n, int b) {
    float2* sx = slot_xy + (size_t)b * per; int* sa = slot_age + (size_t)b * per; int* ss = slot_str + (size_t)b * per;
    const int cap = (b / g.baw) >= g.start_row ? per : 0;                              // feature_set.cpp:113-116
    int cnt = 0;
    for (int i = 0; i < n && cap > 0; i++) {
        const float2 p = xy[i];
        int bh, bw;
        if (!bucket_of(g, p.x, p.y, bh, bw) || bh * g.baw + bw != b) continue;
        const int a = age[i], st = str[i];
        if (a >= g.age_thr) continue;                                                  // :26
        if (cnt < cap) { sx[cnt] = p; sa[cnt] = a; ss[cnt] = st; cnt++; }
        else {
            int smin = bucket_score(sa[0], ss[0], g.fast_thr), imin = 0;
            for (int k = 1; k < cnt; k++) { const int c = bucket_score(sa[k], ss[k], g.fast_thr); if (c < smin) { smin = c; imin = k; } }
            if (bucket_score(a, st, g.fast_thr) > smin) { sx[imin] = p; sa[imin] = a; ss[imin] = st; }
        }
    }
    slot_n[b] = cnt;
}
// The slots of nb buckets in bucket order to out_*[0 .. cap): a block of GEN_EMIT_THREADS threads, each with a run of buckets,
// a block scan of their counts.  Returns the number of filled slots (which may exceed cap) to every thread.
#define GEN_EMIT_THREADS 1024
#define GEN_EMIT_WAVES (GEN_EMIT_THREADS / 64)
static __device__ __forceinline__ int bucket_order_emit(int nb, int per, const float2* slot_xy, const int* slot_age, const int* slot_str, const int* sn,
                                                        int cap, float2* out_xy, int* out_age, int* out_str) {
    __shared__ int wave_tot[GEN_EMIT_WAVES];
    __shared__ int s_total;
    const int chunk = (nb + GEN_EMIT_THREADS - 1) / GEN_EMIT_THREADS;
    const int b0 = threadIdx.x * chunk < nb ? threadIdx.x * chunk : nb, b1 = (b0 + chunk < nb) ? b0 + chunk : nb;
    int cnt = 0;
    for (int b = b0; b < b1; b++) cnt += sn[b];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int incl = cnt;
    for (int o = 1; o < 64; o <<= 1) { int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    if (threadIdx.x == 0) { int acc = 0; for (int i = 0; i < GEN_EMIT_WAVES; i++) { int t = wave_tot[i]; wave_tot[i] = acc; acc += t; } s_total = acc; }
    __syncthreads();
    int pos = wave_tot[wv] + incl - cnt;
    for (int b = b0; b < b1; b++) {
        const size_t so = (size_t)b * per;
        for (int k = 0; k < sn[b]; k++, pos++)
            if (pos < cap) { out_xy[pos] = slot_xy[so + k]; out_age[pos] = slot_age[so + k]; out_str[pos] = slot_str[so + k]; }
    }
    return s_total;
}

// ---- the frame pipeline's wrappers: FAST to the score map (k_fast<2>), the candidate list, the walk, the emit ----
__global__ void k_gen_row_count(DevBuffers d, int pass) {
    const int seq = seq_of(d, blockIdx.y), y = blockIdx.x, W = d.geom.W, H = d.geom.H;
    if (!detect_pass_runs(d.st[seq], pass)) return;
    const int cnt = score_row_count(d.score + ((size_t)seq * H + y) * W, W);
    if (threadIdx.x == 0) d.kp_rows[(size_t)seq * H + y] = cnt;
}
__global__ void k_gen_scan_rows(DevBuffers d, int pass) {          // one lane per sequence
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= launch_seqs(d)) return;
    const int seq = seq_of(d, b);
    SeqState& s = d.st[seq];
    if (!detect_pass_runs(s, pass)) return;
    const int n = scan_rows(d.kp_rows + (size_t)seq * d.geom.H, d.geom.H, s.n_feat);   // keypoints are appended after the existing tracks
    d.n_cand[seq] = n < d.KPCAP ? n : d.KPCAP;
    s.n_old = s.n_feat;
}
__global__ void k_gen_emit_candidates(DevBuffers d, int pass) {
    const int seq = seq_of(d, blockIdx.y), W = d.geom.W, H = d.geom.H;
    const SeqState& s = d.st[seq];
    if (!detect_pass_runs(s, pass)) return;
    float2* cxy = d.cand_xy + (size_t)seq * d.KPCAP; int* cage = d.cand_age + (size_t)seq * d.KPCAP; int* cstr = d.cand_str + (size_t)seq * d.KPCAP;
    if ((int)blockIdx.x == H) {                                      // the extra block copies the existing tracks to the head of the list
        const int fb = s.feat_buf;
        const size_t fo = (size_t)seq * d.CAP;
        for (int i = threadIdx.x; i < s.n_feat; i += 64) { cxy[i] = d.feat_xy[fb][fo + i]; cage[i] = d.feat_age[fb][fo + i]; cstr[i] = d.feat_str[fb][fo + i]; }
        return;
    }
    const int y = blockIdx.x;
    score_row_emit(d.score + ((size_t)seq * H + y) * W, W, d.kp_rows[(size_t)seq * H + y], d.KPCAP,
                   [=](int idx, int x, int sc) { cxy[idx] = make_float2((float)x, (float)y); cage[idx] = 0; cstr[idx] = sc; });   // feature_set.cpp:83-87
}
__global__ void k_gen_bucket_walk(DevBuffers d, int pass) {
    const int seq = seq_of(d, blockIdx.y), b = blockIdx.x * blockDim.x + threadIdx.x, per = d.cfg.features_per_bucket;
    if (b >= d.NB || !detect_pass_runs(d.st[seq], pass)) return;
    const size_t co = (size_t)seq * d.KPCAP, so = (size_t)seq * d.NB * per;
    bucket_walk(grid_of(d), per, d.n_cand[seq], d.cand_xy + co, d.cand_age + co, d.cand_str + co,
                d.slot_xy + so, d.slot_age + so, d.slot_str + so, d.slot_n + (size_t)seq * d.NB, b);
}
__global__ __launch_bounds__(GEN_EMIT_THREADS) void k_gen_bucket_emit(DevBuffers d, int pass) {
    const int seq = seq_of(d, blockIdx.x);
    SeqState& s = d.st[seq];
    if (!detect_pass_runs(s, pass)) return;
    const int fb = s.feat_buf, per = d.cfg.features_per_bucket;
    const size_t so = (size_t)seq * d.NB * per, fo = (size_t)seq * d.CAP;
    const int filled = bucket_order_emit(d.NB, per, d.slot_xy + so, d.slot_age + so, d.slot_str + so, d.slot_n + (size_t)seq * d.NB,
                                         d.CAP, d.feat_xy[fb ^ 1] + fo, d.feat_age[fb ^ 1] + fo, d.feat_str[fb ^ 1] + fo);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = filled < d.CAP ? filled : d.CAP;
        s.n_feat = total; s.feat_buf = fb ^ 1;
        s.stats.n_after_detect = total;
        if (pass == 0) s.do_second = total < d.cfg.pre_matching_feature_threshold;   // vo.cpp:327
        else s.stats.second_pass = 1;
    }
}
static void launch_detect_general(const DevBuffers& d, int pass, int th, hipStream_t st) {
    const int H = d.geom.H, ns = launch_seqs(d);
    hipLaunchKernelGGL(k_fast<2>, fast_grid(d), dim3(256), 0, st, d, pass, th);
    hipLaunchKernelGGL(k_gen_row_count, dim3(H, ns), dim3(64), 0, st, d, pass);
    hipLaunchKernelGGL(k_gen_scan_rows, dim3((ns + 63) / 64), dim3(64), 0, st, d, pass);
    hipLaunchKernelGGL(k_gen_emit_candidates, dim3(H + 1, ns), dim3(64), 0, st, d, pass);
    hipLaunchKernelGGL(k_gen_bucket_walk, dim3((d.NB + 255) / 256, ns), dim3(256), 0, st, d, pass);
    hipLaunchKernelGGL(k_gen_bucket_emit, dim3(ns), dim3(GEN_EMIT_THREADS), 0, st, d, pass);
}

void launch_detect(const DevBuffers& d, int pass, int th_override, hipStream_t st) {
    int th = pass == 0 ? d.cfg.fast_threshold : d.cfg.fast_threshold / 4;            // vo.cpp:325 / :329-330
    if (th_override >= 0) th = th_override;
    if (d.cfg.features_per_bucket > 1) { launch_detect_general(d, pass, th, st); return; }
    // pass 0: k_fast offers the existing tracks itself; pass 1 finds them offered (and n_old set) by the last block of pass 0's emit
    const dim3 g = fast_grid(d);
    static const bool strided_off = getenv("SVO_SECOND_PASS_STRIDED") && atoi(getenv("SVO_SECOND_PASS_STRIDED")) == 0;
    if (pass == 1 && d.B > SVO_LONE_MAX_SEQ && !strided_off) {
        hipLaunchKernelGGL(k_fast_strided, dim3(FAST_STRIDED_BLOCKS, 1, g.z), dim3(256), 0, st, d, pass, th, (int)g.x, (int)g.y);
        hipLaunchKernelGGL(k_bucket_emit_strided, dim3(EMIT_STRIDED_BLOCKS, g.z), dim3(EMIT_THREADS), 0, st, d, pass, d.cfg.buckets_along_height);
        return;
    }
    // pass 0 of a many-sequence context: the batch tile (this launcher serves the contexts without masks and without ids)
    if (d.B > SVO_LONE_MAX_SEQ) hipLaunchKernelGGL(k_fast_batch, dim3(g.x, (d.geom.H + FB_H - 1) / FB_H, g.z), dim3(256), 0, st, d, pass, th);
    else hipLaunchKernelGGL(k_fast<0>, g, dim3(256), 0, st, d, pass, th);
    hipLaunchKernelGGL(k_bucket_emit, dim3(d.cfg.buckets_along_height, g.z), dim3(EMIT_THREADS), 0, st, d, pass);
}

// A detection pass behind masks: the masked FAST kernel of the pass (which offers the filtered tracks itself in pass 0), then the
// plain emit.  Capacity 1 only (svo_set_detection_mask refuses the others).
void launch_detect_masked(const DevBuffers& d, const MaskArgs& m, int pass, int th_override, hipStream_t st) {
    int th = pass == 0 ? d.cfg.fast_threshold : d.cfg.fast_threshold / 4;            // vo.cpp:325 / :329-330
    if (th_override >= 0) th = th_override;
    const dim3 g = fast_grid(d);
    static const bool strided_off = getenv("SVO_SECOND_PASS_STRIDED") && atoi(getenv("SVO_SECOND_PASS_STRIDED")) == 0;
    if (pass == 1 && d.B > SVO_LONE_MAX_SEQ && !strided_off) {
        hipLaunchKernelGGL(k_fast_strided_masked, dim3(FAST_STRIDED_BLOCKS, 1, g.z), dim3(256), 0, st, d, m, pass, th, (int)g.x, (int)g.y);
        hipLaunchKernelGGL(k_bucket_emit_strided, dim3(EMIT_STRIDED_BLOCKS, g.z), dim3(EMIT_THREADS), 0, st, d, pass, d.cfg.buckets_along_height);
        return;
    }
    hipLaunchKernelGGL(k_fast_masked, g, dim3(256), 0, st, d, m, pass, th);
    hipLaunchKernelGGL(k_bucket_emit, dim3(d.cfg.buckets_along_height, g.z), dim3(EMIT_THREADS), 0, st, d, pass);
}

// A detection pass that carries track ids: the pass's FAST kernel — masked when masks are given — then the ids build of the emit.
void launch_detect_ids(const DevBuffers& d, const IdArgs& ia, const MaskArgs* m, int pass, int th_override, hipStream_t st) {
    int th = pass == 0 ? d.cfg.fast_threshold : d.cfg.fast_threshold / 4;            // vo.cpp:325 / :329-330
    if (th_override >= 0) th = th_override;
    const dim3 g = fast_grid(d);
    static const bool strided_off = getenv("SVO_SECOND_PASS_STRIDED") && atoi(getenv("SVO_SECOND_PASS_STRIDED")) == 0;
    if (pass == 1 && d.B > SVO_LONE_MAX_SEQ && !strided_off) {
        if (m) hipLaunchKernelGGL(k_fast_strided_masked, dim3(FAST_STRIDED_BLOCKS, 1, g.z), dim3(256), 0, st, d, *m, pass, th, (int)g.x, (int)g.y);
        else hipLaunchKernelGGL(k_fast_strided, dim3(FAST_STRIDED_BLOCKS, 1, g.z), dim3(256), 0, st, d, pass, th, (int)g.x, (int)g.y);
        hipLaunchKernelGGL(k_bucket_emit_strided_ids, dim3(EMIT_STRIDED_BLOCKS, g.z), dim3(EMIT_THREADS), 0, st, d, ia, pass, d.cfg.buckets_along_height);
        return;
    }
    if (m) hipLaunchKernelGGL(k_fast_masked, g, dim3(256), 0, st, d, *m, pass, th);
    else hipLaunchKernelGGL(k_fast<0>, g, dim3(256), 0, st, d, pass, th);
    hipLaunchKernelGGL(k_bucket_emit_ids, dim3(d.cfg.buckets_along_height, g.z), dim3(EMIT_THREADS), 0, st, d, ia, pass);
}

// ---- the stage call's wrappers (svo_bucket_filter): one grid, the caller's n candidates, n_out = the number emitted ----
__global__ void k_bucket_walk(BucketGrid g, int per, int n, const float2* xy, const int* ages, const int* strs,
                              float2* slot_xy, int* slot_age, int* slot_str, int* slot_n) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < g.bah * g.baw) bucket_walk(g, per, n, xy, ages, strs, slot_xy, slot_age, slot_str, slot_n, b);
}
__global__ __launch_bounds__(GEN_EMIT_THREADS) void k_bucket_order_emit(int nb, int per, const float2* slot_xy, const int* slot_age, const int* slot_str,
                                                                        const int* slot_n, int cap, float2* out_xy, int* out_age, int* out_str, int* n_out) {
    const int filled = bucket_order_emit(nb, per, slot_xy, slot_age, slot_str, slot_n, cap, out_xy, out_age, out_str);
    if (threadIdx.x == 0) *n_out = filled < cap ? filled : cap;
}
void launch_bucket_general(const BucketGrid& g, int per_bucket, int n, const float2* xy, const int* ages, const int* strs,
                           float2* slot_xy, int* slot_age, int* slot_str, int* slot_n,
                           float2* out_xy, int* out_age, int* out_str, int* n_out, hipStream_t st) {
    const int nb = g.bah * g.baw;
    hipLaunchKernelGGL(k_bucket_walk, dim3((nb + 255) / 256), dim3(256), 0, st, g, per_bucket, n, xy, ages, strs, slot_xy, slot_age, slot_str, slot_n);
    hipLaunchKernelGGL(k_bucket_order_emit, dim3(1), dim3(GEN_EMIT_THREADS), 0, st, nb, per_bucket, slot_xy, slot_age, slot_str, slot_n, n,
                       out_xy, out_age, out_str, n_out);
}

// ------------------------------------------------------------------------------------------------
// Stable compaction after circular matching + in-bounds mask (deletePointsWithFailureStatus /
// deleteFeaturesWithFailureStatus, vo.cpp:144-168, called at :233-238 and :360-364), fused with
// ages[i] += 1 (vo.cpp:70-72) and the "too few tracks" gate (vo.cpp:82-84).
// One 256-thread block per sequence, order-preserving prefix sum.
// ------------------------------------------------------------------------------------------------
#define SCAN_THREADS 1024
#define SCAN_WAVES (SCAN_THREADS / 64)
__global__ __launch_bounds__(SCAN_THREADS) void k_compact(DevBuffers d) {
    // One block per sequence walks the tracks in rounds of SCAN_THREADS: coalesced loads, one track per thread, a ballot gives a
    // survivor its rank inside the wave, LDS the survivors of the lower waves, a running total those of the earlier rounds — the
    // output keeps the input order (order is semantics: RANSAC samples rows).  (Round 1: 256 threads x a serial chunk of 8
    // tracks each, two passes of dependent loads: 19 us at one sequence.)
    const int seq = seq_of(d, blockIdx.x);
    SeqState& s = d.st[seq];
    if (!s.active) return;
    __shared__ int sh_cnt[SCAN_WAVES], sh_c[SCAN_WAVES];
    const int n = s.n_lk, fb = s.feat_buf;
    const size_t o = (size_t)seq * d.CAP;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nthr = blockDim.x, nwv = nthr >> 6;                    // 1024 threads for a lone stream (fewest rounds), 256 for many sequences (below)
    const float2* fxy = d.feat_xy[fb] + o; const int* fage = d.feat_age[fb] + o; const int* fstr = d.feat_str[fb] + o;
    float2* nxy = d.feat_xy[fb ^ 1] + o; int* nage = d.feat_age[fb ^ 1] + o; int* nstr = d.feat_str[fb ^ 1] + o;
    int run = 0, cntc = 0;
    unsigned visits = 0, steps = 0;                                  // svo_frame_stats.lk_level_visits / lk_newton_steps
    unsigned dead0 = 0, dead1 = 0, dead2 = 0;                        // svo_frame_stats.lk_dead_after_pass: features that first failed in pass 0, 1, 2
    for (int base = 0; base < n; base += nthr) {
        const int i = base + threadIdx.x;
        uint8_t m = 0;
        if (i < n) {
            m = d.okmask[o + i];
            const unsigned wk = d.lk_work[o + i]; visits += wk & 0x3Fu; steps += wk >> 8;
            const unsigned dk = (wk >> 6) & 3u; dead0 += dk == 1u; dead1 += dk == 2u; dead2 += dk == 3u;
        }
        const bool keep = m == 3;
        cntc += m & 1;
        const unsigned long long bal = __ballot(keep);
        __syncthreads();                                              // the previous round's counts have been read
        if (lane == 0) sh_cnt[wv] = __popcll(bal);
        __syncthreads();
        int pos = run + __popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < nwv; w++) { const int c = sh_cnt[w]; if (w < wv) pos += c; run += c; }
        if (keep) {
            d.tl0[o + pos] = d.pl0[o + i]; d.tl1[o + pos] = d.pl1[o + i];
            d.tr1[o + pos] = d.pr1[o + i]; d.tr0[o + pos] = d.pr0[o + i];
            nxy[pos] = fxy[i]; nage[pos] = fage[i] + 1; nstr[pos] = fstr[i];
        }
    }
    for (int k = 32; k > 0; k >>= 1) { visits += __shfl_xor(visits, k); steps += __shfl_xor(steps, k); cntc += __shfl_xor(cntc, k);
                                     dead0 += __shfl_xor(dead0, k); dead1 += __shfl_xor(dead1, k); dead2 += __shfl_xor(dead2, k); }
    if (lane == 0 && (visits | steps)) { atomicAdd(&s.stats.lk_level_visits, (int)visits); atomicAdd(&s.stats.lk_newton_steps, (int)steps); }
    if (lane == 0 && (dead0 | dead1 | dead2)) {
        atomicAdd(&s.stats.lk_dead_after_pass[0], (int)dead0); atomicAdd(&s.stats.lk_dead_after_pass[1], (int)dead1); atomicAdd(&s.stats.lk_dead_after_pass[2], (int)dead2);
    }
    if (lane == 0) sh_c[wv] = cntc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total_c = 0;
        for (int w = 0; w < nwv; w++) total_c += sh_c[w];
        if (n > 0) {
            s.n_tracks = run; s.n_circ = total_c; s.n_feat = run; s.feat_buf = fb ^ 1;
        } else {
            s.n_tracks = 0; s.n_circ = 0; s.n_feat = 0;           // empty feature set: circularMatching returned early (vo.cpp:179-181)
        }
        int thr = d.cfg.features_threshold > 4 ? d.cfg.features_threshold : 4;
        if (s.n_tracks <= thr) s.fail_reason = 2;                  // vo.cpp:82-84
    }
    // a lone stream's first RANSAC chunk shares a launch with the triangulation (k_tri_epnp): its subsets — a function of the track
    // count alone, which every thread of this block knows by now — are drawn here, one launch earlier, by the first wave
    // (many-sequence contexts: the spare block of k_triangulate)
    if (d.B <= SVO_LONE_MAX_SEQ && wv == 0 && n > 0) {
        const int thr = d.cfg.features_threshold > 4 ? d.cfg.features_threshold : 4;
        if (run > thr && s.active) pnp_draw_first_chunk_wave(d, s, seq, run, pnp_first_chunk(d));
    }
}
void launch_compact(const DevBuffers& d, hipStream_t st) {
    // A 1024-thread block needs four free wave slots on every SIMD of one CU at the same moment.  Beside other resident kernels — the
    // tail of an LK grid, the image stream's kernels of a many-sequence context — that moment comes late: traces show this kernel
    // waiting 0.8-1.6 ms for 20 us of work.  Many-sequence contexts launch it with 256 threads (four times the rounds, no waiting).
    const int threads = d.B > SVO_LONE_MAX_SEQ ? 256 : SCAN_THREADS;
    hipLaunchKernelGGL(k_compact, dim3(launch_seqs(d)), dim3(threads), 0, st, d);
}

// findClosePoints (vo.cpp:265-280) as a stand-alone stage
__global__ void k_find_close(int n, const float2* a, const float2* b, float thr, uint8_t* ok) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float dx = fabsf(a[i].x - b[i].x), dy = fabsf(a[i].y - b[i].y);
    float off = (dx < dy) ? dy : dx;
    ok[i] = off > thr ? 0 : 1;
}
void launch_find_close(int n, const float2* a, const float2* b, float thr, uint8_t* ok, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_find_close, dim3((n + 255) / 256), dim3(256), 0, st, n, a, b, thr, ok);
}

// ------------------------------------------------------------------------------------------------
// Track ids and observation rows (svo.h, svo_set_track_output): the identity rule's steps 2-4 and the two setup kernels.
// ------------------------------------------------------------------------------------------------
// Step 2, behind k_compact: the ids of the features that entered LK through k_compact's stable ranks, recomputed from okmask and
// n_lk with the same ballot scan, to the tracks and to the feature half k_compact has just made current.  One block per launched
// sequence.  (k_compact itself is untouched: its registers and its argument block are what they were.)
#define IDC_THREADS 256
__global__ __launch_bounds__(IDC_THREADS) void k_ids_compact(DevBuffers d, IdArgs a) {
    const int seq = seq_of(d, blockIdx.x);
    const SeqState& s = d.st[seq];
    if (!s.active || s.n_lk <= 0) return;                            // no LK, no compaction: k_compact did not flip the halves
    __shared__ int sh_cnt[IDC_THREADS / 64];
    const int n = s.n_lk, dst = s.feat_buf, src = dst ^ 1;
    const size_t o = (size_t)seq * d.CAP;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long* sid = a.feat_id[src] + o;
    long long* did = a.feat_id[dst] + o; long long* tid = a.track_id + o;
    int run = 0;
    for (int base = 0; base < n; base += IDC_THREADS) {
        const int i = base + threadIdx.x;
        const bool keep = i < n && d.okmask[o + i] == 3;
        const unsigned long long bal = __ballot(keep);
        __syncthreads();                                              // the previous round's counts have been read
        if (lane == 0) sh_cnt[wv] = __popcll(bal);
        __syncthreads();
        int pos = run + __popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < IDC_THREADS / 64; w++) { const int c = sh_cnt[w]; if (w < wv) pos += c; run += c; }
        if (keep) { const long long id = sid[i]; tid[pos] = id; did[pos] = id; }
    }
}
void launch_ids_compact(const DevBuffers& d, const IdArgs& ia, hipStream_t st) {
    hipLaunchKernelGGL(k_ids_compact, dim3(launch_seqs(d)), dim3(IDC_THREADS), 0, st, d, ia);
}

// Steps 3 and 4, behind the pose stage: one block per launched sequence.  Where k_pnp_final replaced the feature set by the inliers
// (fail_reason 0 or 4) new feature pos takes the id of track inl_idx[pos]; then the header and the first min(n_tracks, max_rows)
// rows go straight into the pinned host ring.  A row is 64 bytes = four lanes x 16 bytes: lane 4r + p builds part p of row r in
// registers and a wave stores 1 KiB of consecutive host memory with one dwordx4 store per lane.  Loads and stores only: no LDS.
//   part 0: id, l0     part 1: r0, l1     part 2: r1, xyz[0..1]     part 3: xyz[2], age, flags, pad
#define TO_THREADS 256
static_assert(sizeof(svo_track_obs) == 64, "a row is four 16-byte parts");
static __device__ __forceinline__ void track_obs_body(const DevBuffers& d, const IdArgs& a, const TrackObsArgs& oa) {
    const int seq = seq_of(d, blockIdx.x);
    const SeqState& s = d.st[seq];
    const size_t o = (size_t)seq * d.CAP;
    const int fr = s.fail_reason, fb = s.feat_buf;
    const int n = s.active ? s.n_tracks : 0;
    const bool flipped = n > 0 && (fr == 0 || fr == 4);              // k_pnp_final made the inliers the current half
    if (flipped) {
        long long* nid = a.feat_id[fb] + o;
        const int m = s.n_feat;
        for (int pos = threadIdx.x; pos < m; pos += TO_THREADS) nid[pos] = a.track_id[o + d.inl_idx[o + pos]];
    }
    const int* age = d.feat_age[flipped ? fb ^ 1 : fb] + o;          // step 2's output: position = track index
    const bool has_xyz = fr == 0 || fr == 3 || fr == 4, has_inl = fr == 0 || fr == 4;
    int rows = n < oa.max_rows ? n : oa.max_rows;
    if (rows > d.CAP) rows = d.CAP;
    uint4* out = reinterpret_cast<uint4*>(oa.rows + (size_t)seq * oa.max_rows);
    for (int t = threadIdx.x; t < rows * 4; t += TO_THREADS) {
        const int r = t >> 2, part = t & 3;
        uint4 v;
        if (part == 0) {
            const unsigned long long id = (unsigned long long)a.track_id[o + r];
            const float2 p = d.tl0[o + r];
            v = make_uint4((unsigned)id, (unsigned)(id >> 32), __float_as_uint(p.x), __float_as_uint(p.y));
        } else if (part == 1) {
            const float2 p = d.tr0[o + r], q = d.tl1[o + r];
            v = make_uint4(__float_as_uint(p.x), __float_as_uint(p.y), __float_as_uint(q.x), __float_as_uint(q.y));
        } else if (part == 2) {
            const float2 p = d.tr1[o + r];
            const float* w = d.world + 3 * (o + r);
            v = make_uint4(__float_as_uint(p.x), __float_as_uint(p.y), has_xyz ? __float_as_uint(w[0]) : 0u, has_xyz ? __float_as_uint(w[1]) : 0u);
        } else {
            const unsigned fl = (has_inl && d.inlier[o + r] ? (unsigned)SVO_OBS_INLIER : 0u) | (has_xyz ? (unsigned)SVO_OBS_HAS_XYZ : 0u);
            v = make_uint4(has_xyz ? __float_as_uint(d.world[3 * (o + r) + 2]) : 0u, (unsigned)age[r], fl, 0u);
        }
        out[t] = v;
    }
    if (threadIdx.x == 0) { oa.hdr[2 * seq] = n; oa.hdr[2 * seq + 1] = rows; }
}
// Two builds, as k_pose_cov has: full registers, and the 48-register one a co-resident context launches beside another's LK grid.
__global__ __launch_bounds__(TO_THREADS) void k_track_obs(DevBuffers d, IdArgs a, TrackObsArgs oa) { track_obs_body(d, a, oa); }
__global__ __launch_bounds__(TO_THREADS) __attribute__((amdgpu_num_vgpr(48))) void k_track_obs_lean(DevBuffers d, IdArgs a, TrackObsArgs oa) { track_obs_body(d, a, oa); }
void launch_track_obs(const DevBuffers& d, const IdArgs& ia, const TrackObsArgs& oa, hipStream_t st) {
    hipLaunchKernelGGL(d.co_resident ? k_track_obs_lean : k_track_obs, dim3(launch_seqs(d)), dim3(TO_THREADS), 0, st, d, ia, oa);
}

// Switching the output on: the features every sequence holds get next_id + index, next_id advances by their count.
__global__ __launch_bounds__(256) void k_ids_assign(DevBuffers d, IdArgs a) {
    const int seq = blockIdx.x;
    const SeqState& s = d.st[seq];
    const int n = s.n_feat < d.CAP ? s.n_feat : d.CAP;
    const long long base = a.next_id[seq];
    long long* id = a.feat_id[s.feat_buf] + (size_t)seq * d.CAP;
    for (int i = threadIdx.x; i < n; i += 256) id[i] = base + i;
    __syncthreads();                                                  // every thread has read next_id
    if (threadIdx.x == 0) a.next_id[seq] = base + n;
}
void launch_ids_assign(const DevBuffers& d, const IdArgs& ia, hipStream_t st) {
    hipLaunchKernelGGL(k_ids_assign, dim3(d.B), dim3(256), 0, st, d, ia);
}
__global__ void k_ids_reset(IdArgs a, int seq0, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a.next_id[seq0 + i] = 0;
}
void launch_ids_reset(const IdArgs& ia, int seq0, int n, hipStream_t st) {
    hipLaunchKernelGGL(k_ids_reset, dim3((n + 63) / 64), dim3(64), 0, st, ia, seq0, n);
}
